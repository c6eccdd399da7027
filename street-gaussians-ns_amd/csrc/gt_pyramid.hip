// gt_pyramid.hip — one pyramid level of a batch's byte ground truth for coarse-to-fine training, gfx950.
//
// The reference trains coarse to fine: while d = 2 ** max(num_downscales - step // resolution_schedule, 0) > 1 it
// resizes the batch's image with TF.resize(..., antialias=None) — plain bilinear, align_corners=False — and the mask
// and the semantic map with InterpolationMode.NEAREST (sgn_splatfacto.py:766-784, :822-823, :1055-1071).  One launch
// here reads the uint8 image [h,w,3] and the optional uint8 mask / semantic map [h,w] as the feed caches them and
// writes the float32 image [oh,ow,3] and the mask / semantic bytes [oh,ow] of the level; no float image of the full
// resolution is ever materialised.
//
// Arithmetic contract (tests/pyramid_oracle.py restates it operation for operation; the library is built with
// -ffp-contract=off, so nothing below fuses into an FMA).  fp32 throughout, per axis (in -> out):
//   scale = (float)in / (float)out                        a true fp32 division (formed on the host, IEEE)
//   src   = max(scale * ((float)dst + 0.5f) - 0.5f, 0.0f)
//   i0    = min((int)src, in - 1)
//   i1    = i0 + (i0 < in - 1)
//   l1    = src - (float)i0
//   l0    = 1.0f - l1
//   out   = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)     per channel; a, b on row i0h; a, c on column i0w
//   a..d  = the correctly rounded (float)u / 255.0f of the four bytes: sgn_byte_unorm, the quotient the byte loss forms
//   nearest (mask, semantic): min((int)floorf((float)dst * scale), in - 1) per axis; the source byte unchanged
//
// A streaming kernel: one workgroup per 256-pixel segment of one output row, consecutive lanes on consecutive output
// pixels, so everything that depends on the row only (both source rows, their weights, the nearest row, all row
// offsets) is wave-uniform and stays in scalar registers.  No LDS, no atomics, no workspace.  h, w <= 16384: every
// element index is below 2^31 (16384 * 16384 * 3 = 805 306 368).
#include "sgn_common.h"

namespace {

struct Taps { int i0, i1; float l0, l1; };

__device__ __forceinline__ Taps bilinear_taps(int dst, float scale, int in) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    Taps t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__device__ __forceinline__ int nearest_index(int dst, float scale, int in) {
    return min((int)floorf((float)dst * scale), in - 1);
}

constexpr int BLOCK = 256;

// grid (ceil(ow / 256), oh); mask / semantic NULL: that map is absent (wave-uniform branches)
__global__ __launch_bounds__(BLOCK) void gt_downscale_kernel(int h, int w, int ow, float scale_h, float scale_w,
                                                             const unsigned char *__restrict__ image,
                                                             const unsigned char *__restrict__ mask,
                                                             const unsigned char *__restrict__ semantic,
                                                             float *__restrict__ image_out,
                                                             unsigned char *__restrict__ mask_out,
                                                             unsigned char *__restrict__ semantic_out) {
    const int y = blockIdx.y;                                  // the row: uniform, so is everything derived from it
    const Taps ty = bilinear_taps(y, scale_h, h);
    const unsigned char *row0 = image + ty.i0 * w * 3, *row1 = image + ty.i1 * w * 3;
    const int near_row = nearest_index(y, scale_h, h) * w;
    const int x = blockIdx.x * BLOCK + threadIdx.x;
    if (x >= ow) return;
    const Taps tx = bilinear_taps(x, scale_w, w);
    const int c0 = tx.i0 * 3, c1 = tx.i1 * 3;
    unsigned char a[3], b[3], c[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                              // the twelve byte loads, all issued before the arithmetic
        a[k] = row0[c0 + k]; b[k] = row0[c1 + k];
        c[k] = row1[c0 + k]; d[k] = row1[c1 + k];
    }
    const int o = y * ow + x;
    if (mask || semantic) {
        const int n = near_row + nearest_index(x, scale_w, w);
        if (mask) mask_out[o] = mask[n];
        if (semantic) semantic_out[o] = semantic[n];
    }
    float *out = image_out + o * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = tx.l0 * sgn_byte_unorm(a[k]) + tx.l1 * sgn_byte_unorm(b[k]);
        const float bot = tx.l0 * sgn_byte_unorm(c[k]) + tx.l1 * sgn_byte_unorm(d[k]);
        out[k] = ty.l0 * top + ty.l1 * bot;
    }
}

}  // namespace

int sgn_gt_downscale_launch(int h, int w, int oh, int ow, const unsigned char *image, const unsigned char *mask,
                            const unsigned char *semantic, float *image_out, unsigned char *mask_out,
                            unsigned char *semantic_out, sgn_stream_t stream) {
    const float scale_h = (float)h / (float)oh, scale_w = (float)w / (float)ow;
    hipLaunchKernelGGL(gt_downscale_kernel, dim3(sgn_cdiv(ow, BLOCK), oh), dim3(BLOCK), 0, (hipStream_t)stream, h, w, ow,
                       scale_h, scale_w, image, mask, semantic, image_out, mask_out, semantic_out);
    SGN_LAUNCH_CHECK();
    return 0;
}
