// frame_pack.hip — a frame's eval outputs as the bytes an image or video writer takes, gfx950.
//
// The reference's render script (scripts/render.py:159-273) runs every output of every frame through
// colormaps.apply_colormap / apply_depth_colormap, moves the float32 result to the host and leaves the float -> uint8
// conversion to the writer: nine float32 images across PCIe per frame.  One launch here reads up to 16 panels of one
// frame — float32 [h,w,3], float32 [h,w] with a 256-row colour table, or uint8 [h,w,3] — and writes their bytes into
// rectangles of one uint8 canvas [canvas_h, canvas_w, 3]; a quarter of the bytes then cross, once (sgn_rast/frames.py).
//
// Arithmetic contract (include/sgn_rast.h; tests/frames_oracle.py restates it operation for operation; the library is
// built with -ffp-contract=off, so the multiply and the add below stay two roundings).  fp32 throughout:
//   unit(v) = v > 0 ? (v < 1 ? v : 1) : 0                  clamp to [0, 1]; NaN -> 0, -inf -> 0, +inf -> 1
//   RGB     byte = (uint8) trunc(unit(x) * 255.0f + 0.5f)   per channel
//   SCALAR  t = unit((x - lo) / den)                        IEEE division; clip with NaN propagating, then NaN -> 0
//           t = 1 - t if invert;  bytes = lut[(int) trunc(t * 255.0f)]
//   BYTES   copied
//
// A streaming kernel: grid (ceil(ceil(w / 4) / 256), h, n_panels); a workgroup has one 1024-pixel segment of one row of
// one panel, a lane four consecutive pixels of it.  The panel table travels by value in the kernel arguments and is
// indexed by blockIdx.z, so a panel's fields, the row and every branch on them are wave-uniform.  Where the quads are
// aligned (w, x0 and canvas_w multiples of 4, a 16-byte aligned float source or a 4-byte aligned byte source, a 4-byte
// aligned canvas) a lane reads its quad with 16-byte loads (three for RGB, one for SCALAR; three dwords for BYTES) and
// writes its 12 bytes as three dwords; otherwise it goes pixel by pixel, byte by byte, and bounds its quad by w.  Both
// paths form the same bytes.  The colour table of a SCALAR panel is staged in LDS as one dword per row (1 KiB): one LDS
// read per pixel.  No scratch, no atomics, no workspace.  h, w, canvas_h, canvas_w <= 16384: every element index is
// below 2^31 (16384 * 16384 * 3 = 805 306 368).
#include "sgn_common.h"

namespace {

constexpr int BLOCK = 256;      // == the rows of a colour table: lane i stages row i

struct PanelTable { sgn_panel p[SGN_FRAMES_MAX_PANELS]; };

__device__ __forceinline__ float unit_clamp(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }

// one pixel's three bytes as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t rgb_triple(float r, float g, float b) {
    const uint32_t qr = (uint32_t)(unit_clamp(r) * 255.0f + 0.5f);
    const uint32_t qg = (uint32_t)(unit_clamp(g) * 255.0f + 0.5f);
    const uint32_t qb = (uint32_t)(unit_clamp(b) * 255.0f + 0.5f);
    return qr | (qg << 8) | (qb << 16);
}

__device__ __forceinline__ int lut_row(float x, float lo, float den, int invert) {
    float t = unit_clamp(__fdiv_rn(x - lo, den));
    if (invert) t = 1.0f - t;
    return (int)(t * 255.0f);
}

__device__ __forceinline__ void store_triple(unsigned char *dst, uint32_t t) {
    dst[0] = (unsigned char)t; dst[1] = (unsigned char)(t >> 8); dst[2] = (unsigned char)(t >> 16);
}

__global__ __launch_bounds__(BLOCK) void frames_pack_kernel(int w, int canvas_w, unsigned char *__restrict__ canvas,
                                                            const PanelTable table) {
    __shared__ uint32_t lut_s[BLOCK];
    const sgn_panel &p = table.p[blockIdx.z];                  // uniform: scalar loads from the kernel arguments
    const int kind = p.kind;
    if (kind == SGN_PANEL_SCALAR) {                            // uniform branch: the whole workgroup takes the barrier
        const unsigned char *row = p.lut + threadIdx.x * 3;
        lut_s[threadIdx.x] = (uint32_t)row[0] | ((uint32_t)row[1] << 8) | ((uint32_t)row[2] << 16);
        __syncthreads();
    }
    const int y = blockIdx.y;
    const int x = (blockIdx.x * BLOCK + threadIdx.x) * 4;      // the lane's quad: pixels x .. x + 3 of row y
    if (x >= w) return;
    const int pix = y * w + x;
    unsigned char *dst = canvas + ((p.y0 + y) * canvas_w + p.x0 + x) * 3;
    const uintptr_t src_align = kind == SGN_PANEL_BYTES ? 3 : 15;
    const bool quads = ((w | p.x0 | canvas_w) & 3) == 0 && ((uintptr_t)p.src & src_align) == 0 &&
                       ((uintptr_t)canvas & 3) == 0;           // uniform
    if (quads) {                                               // w % 4 == 0: the quad is whole
        uint32_t *out = reinterpret_cast<uint32_t *>(dst);     // (row * canvas_w + x0 + x) * 3 is a multiple of 12
        if (kind == SGN_PANEL_BYTES) {
            const uint32_t *s = reinterpret_cast<const uint32_t *>((const unsigned char *)p.src + pix * 3);
            const uint32_t a = s[0], b = s[1], c = s[2];
            out[0] = a; out[1] = b; out[2] = c;
            return;
        }
        uint32_t t0, t1, t2, t3;
        if (kind == SGN_PANEL_RGB) {
            const float4 *s = reinterpret_cast<const float4 *>((const float *)p.src + pix * 3);
            const float4 a = s[0], b = s[1], c = s[2];
            t0 = rgb_triple(a.x, a.y, a.z); t1 = rgb_triple(a.w, b.x, b.y);
            t2 = rgb_triple(b.z, b.w, c.x); t3 = rgb_triple(c.y, c.z, c.w);
        } else {
            const float4 v = *reinterpret_cast<const float4 *>((const float *)p.src + pix);
            t0 = lut_s[lut_row(v.x, p.lo, p.den, p.invert)]; t1 = lut_s[lut_row(v.y, p.lo, p.den, p.invert)];
            t2 = lut_s[lut_row(v.z, p.lo, p.den, p.invert)]; t3 = lut_s[lut_row(v.w, p.lo, p.den, p.invert)];
        }
        out[0] = t0 | (t1 << 24);
        out[1] = (t1 >> 8) | (t2 << 16);
        out[2] = (t2 >> 16) | (t3 << 8);
        return;
    }
    const int n = min(4, w - x);                               // a row's tail, w < 4
    for (int i = 0; i < n; ++i) {
        uint32_t t;
        if (kind == SGN_PANEL_BYTES) {
            const unsigned char *s = (const unsigned char *)p.src + (pix + i) * 3;
            t = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        } else if (kind == SGN_PANEL_RGB) {
            const float *s = (const float *)p.src + (pix + i) * 3;
            t = rgb_triple(s[0], s[1], s[2]);
        } else {
            t = lut_s[lut_row(((const float *)p.src)[pix + i], p.lo, p.den, p.invert)];
        }
        store_triple(dst + i * 3, t);
    }
}

}  // namespace

int sgn_frames_pack_launch(int h, int w, int n_panels, const sgn_panel *panels, unsigned char *canvas, int canvas_w,
                           sgn_stream_t stream) {
    PanelTable table = {};
    for (int i = 0; i < n_panels; ++i) table.p[i] = panels[i];
    hipLaunchKernelGGL(frames_pack_kernel, dim3(sgn_cdiv(sgn_cdiv(w, 4), BLOCK), h, n_panels), dim3(BLOCK), 0,
                       (hipStream_t)stream, w, canvas_w, canvas, table);
    SGN_LAUNCH_CHECK();
    return 0;
}
