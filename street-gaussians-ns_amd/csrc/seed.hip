// seed.hip — LiDAR seeding of the scene graph's Gaussians: one sweep against one camera and up to 64 boxes, gfx950.
//
// The reference colours LiDAR points from the camera image they project into and sorts them into the background cloud
// (scripts/pythons/pcd2colmap_points3D.py:114-235: points outside every moving box, world frame) and one cloud per
// tracked object (scripts/pythons/extract_object_pts.py:114-273: points inside the box scaled 1.1, box frame), with a
// Python loop over every point and open3d's box test.  Here it is a classification and a stable partition:
//   classify  one lane per point: live / visible, a 64-bit box membership word, the pixel, and per 256-point block one
//             count per destination (64 boxes, background, live) from __popcll(__ballot(..)), plain stores;
//   scan      one workgroup per destination turns its column of block counts into exclusive offsets and a total;
//   emit      one lane per point again: ranks inside the wave by ballot + mbcnt, inside the block through LDS, and
//             writes every destination's rows in input order.
// No atomics anywhere: every output is stable and bit-identical from run to run.  The arithmetic is a contract
// (include/sgn_rast.h "LiDAR SEEDING"): fp32, the parenthesisation written there, IEEE division, no contraction
// (-ffp-contract=off on every translation unit), so a float32 restatement reproduces every output bit for bit.
#include "sgn_common.h"

namespace {

constexpr int SD_BLOCK = 256;                       // points per workgroup (the unit of the block counts)
constexpr int SD_WAVES = SD_BLOCK / 64;
constexpr int SD_MAX_DEST = SGN_SEED_MAX_BOXES + 2; // boxes, background, live
constexpr int SD_BOX_FLOATS = 15;                   // center[3], rot[9], half[3]
constexpr int SD_CHUNK_BOXES = 16;                  // boxes per upload launch: 960 bytes of kernel arguments
constexpr int SD_HEAD_FLOATS = 64;                  // l2w[12] in front of the box table, padded to 256 bytes
constexpr uint32_t PIX_OK = 1u << 28;               // live & visible; u in bits 0-13, v in bits 14-27 (W, H <= 16384)

struct SeedHead { float l2w[12]; };
struct SeedChunk { float v[SD_CHUNK_BOXES * SD_BOX_FLOATS]; };
struct SeedCamArgs { float V[12]; float fx, fy, cx, cy, min_z; int W, H; };

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int n_blocks(int n) { return sgn_cdiv(n, SD_BLOCK); }
inline size_t ws_table_bytes() { return al256((SD_HEAD_FLOATS + SGN_SEED_MAX_BOXES * SD_BOX_FLOATS) * sizeof(float)); }
inline size_t ws_member_bytes(int n) { return al256((size_t)n * sizeof(uint64_t)); }
inline size_t ws_pix_bytes(int n) { return al256((size_t)n * sizeof(uint32_t)); }
inline size_t ws_blk_bytes(int n, int n_boxes) { return al256((size_t)n_blocks(n) * (n_boxes + 2) * sizeof(int32_t)); }
inline size_t ws_totals_bytes() { return al256(SD_MAX_DEST * sizeof(int32_t)); }

struct SeedWs {
    float *head, *boxes;
    uint64_t *member;
    uint32_t *pix;
    int32_t *blk, *totals;
};
inline SeedWs carve(void *ws, int n, int n_boxes) {
    char *p = (char *)ws;
    SeedWs w;
    w.head = (float *)p; w.boxes = w.head + SD_HEAD_FLOATS; p += ws_table_bytes();
    w.member = (uint64_t *)p; p += ws_member_bytes(n);
    w.pix = (uint32_t *)p; p += ws_pix_bytes(n);
    w.blk = (int32_t *)p; p += ws_blk_bytes(n, n_boxes);
    w.totals = (int32_t *)p;
    return w;
}

// M (3x4 row-major) applied to (x, y, z): ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]
__device__ __forceinline__ void affine(const float *__restrict__ M, float x, float y, float z, float &ox, float &oy,
                                       float &oz) {
    ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

// the point in box b's frame: loc[k] = (R[0][k] d0 + R[1][k] d1) + R[2][k] d2, d = pw - center (box = 15 floats)
__device__ __forceinline__ void box_local(const float *__restrict__ box, float wx, float wy, float wz, float &l0,
                                          float &l1, float &l2) {
    const float d0 = wx - box[0], d1 = wy - box[1], d2 = wz - box[2];
    const float *R = box + 3;
    l0 = (R[0] * d0 + R[3] * d1) + R[6] * d2;
    l1 = (R[1] * d0 + R[4] * d1) + R[7] * d2;
    l2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
}

__device__ __forceinline__ int lane_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The host's tables into the workspace: l2w (with the first chunk) and `count` boxes from box `first` on.
__global__ __launch_bounds__(256) void seed_upload_kernel(SeedHead head, SeedChunk chunk, int first, int count,
                                                          float *__restrict__ head_out, float *__restrict__ boxes_out) {
    const int t = threadIdx.x;
    if (first == 0 && t < 12) head_out[t] = head.l2w[t];
    if (t < count * SD_BOX_FLOATS) boxes_out[first * SD_BOX_FLOATS + t] = chunk.v[t];
}

__global__ __launch_bounds__(SD_BLOCK) void seed_classify_kernel(int n, int n_boxes, int nblk,
                                                                 const float *__restrict__ points, SeedCamArgs C,
                                                                 const float *__restrict__ head,
                                                                 const float *__restrict__ boxes,
                                                                 uint64_t *__restrict__ member,
                                                                 uint32_t *__restrict__ pix, int32_t *__restrict__ blk) {
    __shared__ int32_t wcnt[SD_WAVES][SD_MAX_DEST];
    const int i = blockIdx.x * SD_BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool live = false, ok = false;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    uint32_t word = 0u;
    if (i < n) {
        const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
        live = !(x != x || y != y || z != z) && z > C.min_z;
        affine(head, x, y, z, wx, wy, wz);
        live = live && !(fabsf(wx) > 1e5f);
        float cx_, cy_, cz_;
        affine(C.V, wx, wy, wz, cx_, cy_, cz_);
        const float fu = (C.fx * cx_ + C.cx * cz_) / cz_, fv = (C.fy * cy_ + C.cy * cz_) / cz_;
        // trunc(fu) in [0, W) <=> -1 < fu < W (W <= 16384 is exact in fp32); NaN and inf fail a comparison
        const bool vis = cz_ > 0.f && fu > -1.f && fu < (float)C.W && fv > -1.f && fv < (float)C.H;
        ok = live && vis;
        if (ok) word = PIX_OK | (uint32_t)(int)fu | ((uint32_t)(int)fv << 14);
    }
    uint64_t in = 0ull;
    for (int b = 0; b < n_boxes; ++b) {             // wave-uniform: the box table is read through scalar loads
        const float *box = boxes + b * SD_BOX_FLOATS;
        float l0, l1, l2;
        box_local(box, wx, wy, wz, l0, l1, l2);
        const bool in_b = ok && fabsf(l0) <= box[12] && fabsf(l1) <= box[13] && fabsf(l2) <= box[14];
        const unsigned long long m = __ballot(in_b);
        if (lane == 0) wcnt[wave][b] = __popcll(m);
        if (in_b) in |= 1ull << b;
    }
    const unsigned long long m_bg = __ballot(ok && in == 0ull), m_live = __ballot(live);
    if (lane == 0) { wcnt[wave][n_boxes] = __popcll(m_bg); wcnt[wave][n_boxes + 1] = __popcll(m_live); }
    if (i < n) { member[i] = in; pix[i] = word; }
    __syncthreads();
    if ((int)threadIdx.x < n_boxes + 2) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < SD_WAVES; ++w) s += wcnt[w][threadIdx.x];
        blk[(size_t)threadIdx.x * nblk + blockIdx.x] = s;    // column-major: one contiguous column per destination
    }
}

// One workgroup per destination: its column of block counts becomes the exclusive sums over the blocks before, its total
// goes to both totals arrays.  Thread t owns the blocks [t * per, (t + 1) * per); integer sums in a fixed order.
__global__ __launch_bounds__(256) void seed_scan_kernel(int nblk, int32_t *__restrict__ blk,
                                                        int32_t *__restrict__ totals_ws, int32_t *__restrict__ totals_out) {
    __shared__ int32_t part[256];
    int32_t *col = blk + (size_t)blockIdx.x * nblk;
    const int per = (nblk + 255) / 256;
    const int b0 = min((int)threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
    int32_t acc = 0;
    for (int b = b0; b < b1; ++b) acc += col[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int t = 0; t < 256; ++t) { const int32_t v = part[t]; part[t] = run; run += v; }
        totals_ws[blockIdx.x] = run;
        totals_out[blockIdx.x] = run;
    }
    __syncthreads();
    int32_t run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) { const int32_t v = col[b]; col[b] = run; run += v; }
}

__global__ __launch_bounds__(SD_BLOCK) void seed_emit_kernel(
    int n, int n_boxes, int nblk, const float *__restrict__ points, const uint8_t *__restrict__ image, int W, int H,
    const float *__restrict__ head, const float *__restrict__ boxes, const uint64_t *__restrict__ member,
    const uint32_t *__restrict__ pix, const int32_t *__restrict__ blk, const int32_t *__restrict__ totals,
    float *__restrict__ obj_xyz, uint8_t *__restrict__ obj_rgb, int32_t *__restrict__ obj_src, long long obj_cap,
    float *__restrict__ bg_xyz, uint8_t *__restrict__ bg_rgb, int32_t *__restrict__ bg_src, long long bg_cap) {
    __shared__ int32_t wcnt[SD_WAVES][SGN_SEED_MAX_BOXES + 1];
    __shared__ long long base[SGN_SEED_MAX_BOXES];  // first object row of every box: exclusive sums of the box totals
    const int i = blockIdx.x * SD_BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t in = i < n ? member[i] : 0ull;
    const uint32_t word = i < n ? pix[i] : 0u;
    const bool ok = (word & PIX_OK) != 0u;
    const bool bg = ok && in == 0ull;
    for (int b = 0; b < n_boxes; ++b) {
        const unsigned long long m = __ballot((in >> b) & 1ull);
        if (lane == 0) wcnt[wave][b] = __popcll(m);
    }
    const unsigned long long m_bg = __ballot(bg);
    if (lane == 0) wcnt[wave][n_boxes] = __popcll(m_bg);
    if (threadIdx.x < 64) {                         // wave 0, whole
        const long long v = lane < n_boxes ? (long long)totals[lane] : 0ll;
        long long inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        base[lane] = inc - v;
    }
    __syncthreads();
    float wx = 0.f, wy = 0.f, wz = 0.f;
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if (ok) {
        affine(head, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], wx, wy, wz);
        const int u = (int)(word & 0x3fffu), v = (int)((word >> 14) & 0x3fffu);
        if (u < W && v < H) {                       // always, for the image size classify saw
            const uint8_t *px = image + ((size_t)v * W + u) * 3;
            c0 = px[0]; c1 = px[1]; c2 = px[2];
        }
    }
    for (int b = 0; b < n_boxes; ++b) {
        const bool mine = (in >> b) & 1ull;
        const unsigned long long m = __ballot(mine);
        if (m == 0ull) continue;                    // wave-uniform
        long long r = base[b] + blk[(size_t)b * nblk + blockIdx.x];
        for (int w = 0; w < wave; ++w) r += wcnt[w][b];
        r += lane_rank(m);
        if (mine && r < obj_cap) {
            float l0, l1, l2;
            box_local(boxes + b * SD_BOX_FLOATS, wx, wy, wz, l0, l1, l2);
            obj_xyz[3 * r] = l0; obj_xyz[3 * r + 1] = l1; obj_xyz[3 * r + 2] = l2;
            obj_rgb[3 * r] = c0; obj_rgb[3 * r + 1] = c1; obj_rgb[3 * r + 2] = c2;
            obj_src[r] = i;
        }
    }
    if (m_bg != 0ull) {
        long long r = blk[(size_t)n_boxes * nblk + blockIdx.x];
        for (int w = 0; w < wave; ++w) r += wcnt[w][n_boxes];
        r += lane_rank(m_bg);
        if (bg && r < bg_cap) {
            bg_xyz[3 * r] = wx; bg_xyz[3 * r + 1] = wy; bg_xyz[3 * r + 2] = wz;
            bg_rgb[3 * r] = c0; bg_rgb[3 * r + 1] = c1; bg_rgb[3 * r + 2] = c2;
            bg_src[r] = i;
        }
    }
}

}  // namespace

SGN_EXPORT size_t sgn_seed_workspace_bytes(int n, int n_boxes) {
    if (n < 1 || n > SGN_SEED_MAX_POINTS || n_boxes < 0 || n_boxes > SGN_SEED_MAX_BOXES) return 0;
    return ws_table_bytes() + ws_member_bytes(n) + ws_pix_bytes(n) + ws_blk_bytes(n, n_boxes) + ws_totals_bytes();
}

SGN_EXPORT int sgn_seed_classify(int n, const float *points, const float *l2w12, float min_z, int n_boxes,
                                 const sgn_seed_box *boxes, const sgn_seed_cam *cam, void *ws, size_t ws_bytes,
                                 int32_t *totals, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 1 && n <= SGN_SEED_MAX_POINTS, -1);
    SGN_ARG_CHECK(n_boxes >= 0 && n_boxes <= SGN_SEED_MAX_BOXES, -2);
    SGN_ARG_CHECK(cam != nullptr, -4);
    SGN_ARG_CHECK(cam->width >= 1 && cam->width <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(cam->height >= 1 && cam->height <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(points != nullptr, -4);
    SGN_ARG_CHECK(l2w12 != nullptr, -4);
    SGN_ARG_CHECK(n_boxes == 0 || boxes != nullptr, -4);
    SGN_ARG_CHECK(ws != nullptr, -4);
    SGN_ARG_CHECK(totals != nullptr, -4);
    SGN_ARG_CHECK(ws_bytes >= sgn_seed_workspace_bytes(n, n_boxes), -5);
    hipStream_t s = (hipStream_t)stream;
    const SeedWs w = carve(ws, n, n_boxes);
    SeedHead head;
    for (int k = 0; k < 12; ++k) head.l2w[k] = l2w12[k];
    for (int first = 0; first == 0 || first < n_boxes; first += SD_CHUNK_BOXES) {
        const int count = n_boxes - first < SD_CHUNK_BOXES ? n_boxes - first : SD_CHUNK_BOXES;
        SeedChunk chunk = {};
        for (int b = 0; b < count; ++b) {
            const sgn_seed_box &B = boxes[first + b];
            float *o = chunk.v + b * SD_BOX_FLOATS;
            for (int k = 0; k < 3; ++k) o[k] = B.center[k];
            for (int k = 0; k < 9; ++k) o[3 + k] = B.rot[k];
            for (int k = 0; k < 3; ++k) o[12 + k] = B.half[k];
        }
        hipLaunchKernelGGL(seed_upload_kernel, dim3(1), dim3(256), 0, s, head, chunk, first, count, w.head, w.boxes);
    }
    SeedCamArgs C;
    for (int k = 0; k < 12; ++k) C.V[k] = cam->w2c[k];
    C.fx = cam->fx; C.fy = cam->fy; C.cx = cam->cx; C.cy = cam->cy; C.min_z = min_z;
    C.W = cam->width; C.H = cam->height;
    const int nblk = n_blocks(n);
    hipLaunchKernelGGL(seed_classify_kernel, dim3(nblk), dim3(SD_BLOCK), 0, s, n, n_boxes, nblk, points, C, w.head,
                       w.boxes, w.member, w.pix, w.blk);
    hipLaunchKernelGGL(seed_scan_kernel, dim3(n_boxes + 2), dim3(256), 0, s, nblk, w.blk, w.totals, totals);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_seed_emit(int n, const float *points, int n_boxes, const uint8_t *image, int width, int height,
                             const void *ws, size_t ws_bytes, float *obj_local, uint8_t *obj_rgb, int32_t *obj_src,
                             int64_t obj_rows, float *bg_world, uint8_t *bg_rgb, int32_t *bg_src, int64_t bg_rows,
                             sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 1 && n <= SGN_SEED_MAX_POINTS, -1);
    SGN_ARG_CHECK(n_boxes >= 0 && n_boxes <= SGN_SEED_MAX_BOXES, -2);
    SGN_ARG_CHECK(width >= 1 && width <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(height >= 1 && height <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(obj_rows >= 0 && obj_rows <= (int64_t)n * SGN_SEED_MAX_BOXES, -6);
    SGN_ARG_CHECK(bg_rows >= 0 && bg_rows <= (int64_t)n, -6);
    SGN_ARG_CHECK(points != nullptr, -4);
    SGN_ARG_CHECK(image != nullptr, -4);
    SGN_ARG_CHECK(ws != nullptr, -4);
    SGN_ARG_CHECK(obj_rows == 0 || (obj_local && obj_rgb && obj_src), -4);
    SGN_ARG_CHECK(bg_rows == 0 || (bg_world && bg_rgb && bg_src), -4);
    SGN_ARG_CHECK(ws_bytes >= sgn_seed_workspace_bytes(n, n_boxes), -5);
    if (obj_rows == 0 && bg_rows == 0) return 0;
    const SeedWs w = carve(const_cast<void *>(ws), n, n_boxes);
    const int nblk = n_blocks(n);
    hipLaunchKernelGGL(seed_emit_kernel, dim3(nblk), dim3(SD_BLOCK), 0, (hipStream_t)stream, n, n_boxes, nblk, points,
                       image, width, height, w.head, w.boxes, w.member, w.pix, w.blk, w.totals, obj_local, obj_rgb,
                       obj_src, (long long)obj_rows, bg_world, bg_rgb, bg_src, (long long)bg_rows);
    SGN_LAUNCH_CHECK();
    return 0;
}
