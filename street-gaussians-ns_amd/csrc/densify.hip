// densify.hip — the refinement itself (split / duplicate / cull + the optimiser-state surgery) as fused passes, gfx950.
//
// SplatfactoModel.refinement_after / split_gaussians / dup_gaussians / cull_gaussians / dup_in_optim /
// remove_from_optim (street_gaussians_ns/sgn_splatfacto.py:459-720) as sgn_rast.densify.Densifier's torch engine
// restates them, decision for decision and row for row:
//   decide  one lane per INPUT Gaussian: a flag byte and, per 256-row block, eight integer sums;
//   scan    one workgroup turns the block sums into exclusive offsets and the totals the host reads back once;
//   apply   a row map (src / kind of every OUTPUT row) and then ONE table-driven launch that writes every new
//           parameter and Adam-moment tensor at its final size straight from the inputs.
// Everything about one Gaussian's fate is a function of its own input row (every child of a parent shares the
// parent's verdict), so no [old, children, dups] array is ever materialised.  Integer sums only, no atomics at all:
// replicas under data parallelism stay bit-identical.  Built with -ffp-contract=off and without fast-math: x/0 = inf
// is "high", 0/0 = NaN is not, as in torch.
#include "sgn_common.h"

namespace {

constexpr int DN_BLOCK = 256;               // rows per workgroup of decide / map (the unit of the block sums)
constexpr int DN_SUMS = 8;                  // ints per block: keep, split, kids, dup_keep | high, dups, toobig, -
constexpr int DN_TOTALS = 8;                // kept originals, split parents, kept split parents, kept dups | the same 4
constexpr int DN_MAX_TENSORS = 24;
constexpr int DN_CHUNK = 256 * 4 * 4;       // output elements per workgroup of apply: 256 threads x 4 x float4

enum : unsigned { F_KEEP = 1u, F_SPLIT = 2u, F_KIDS = 4u, F_DUPKEEP = 8u, F_HIGH = 16u, F_DUP = 32u };
enum { ROLE_COPY = 0, ROLE_MEANS = 1, ROLE_LOG_SCALES = 2, ROLE_MOMENT = 3 };

struct DecideArgs {
    float grad_thresh, size_thresh, split_screen, cull_alpha, cull_scale, cull_screen, dim;
    int samps, densify, screen_on, toobig_on;
};

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t ws_flags_bytes(int n) { return al256((size_t)n); }
inline size_t ws_blk_bytes(int n) { return al256((size_t)sgn_cdiv(n, DN_BLOCK) * DN_SUMS * sizeof(int32_t)); }

// torch.max over a dimension propagates NaN; fmaxf does not
__device__ __forceinline__ float max3_nan(float a, float b, float c) {
    if (a != a || b != b || c != c) return __builtin_nanf("");
    return fmaxf(fmaxf(a, b), c);
}
__device__ __forceinline__ float shrink(float log_scale) { return logf(expf(log_scale) / 1.6f); }

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(DN_BLOCK) void densify_decide_kernel(
    int n, const float *__restrict__ grad_norm, const float *__restrict__ vis_counts,
    const float *__restrict__ max_2dsize, const float *__restrict__ log_scales, const float *__restrict__ opacity,
    DecideArgs A, uint8_t *__restrict__ flags, int32_t *__restrict__ blk) {
    __shared__ int32_t wsum[DN_BLOCK / 64][DN_SUMS];
    const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
    const bool live = i < n;
    bool keep = false, split = false, kids = false, dup_keep = false, high = false, dup = false;
    bool tb_self = false, tb_kids = false, tb_dup = false;
    if (live) {
        const float l0 = log_scales[3 * (size_t)i], l1 = log_scales[3 * (size_t)i + 1], l2 = log_scales[3 * (size_t)i + 2];
        const float size = max3_nan(expf(l0), expf(l1), expf(l2));
        const float m2d = A.screen_on ? max_2dsize[i] : 0.f;
        float size_now = size;                  // the scale the duplicate / cull tests see: shrunk for a split parent
        if (A.densify) {
            const float avg = (grad_norm[i] / vis_counts[i]) * 0.5f * A.dim;
            high = avg > A.grad_thresh;
            split = size > A.size_thresh;
            if (A.screen_on) split = split || (m2d > A.split_screen);
            split = split && high;
            if (split) size_now = max3_nan(expf(shrink(l0)), expf(shrink(l1)), expf(shrink(l2)));
            dup = (size_now <= A.size_thresh) && high;
        }
        const bool alpha = (1.f / (1.f + expf(-opacity[i]))) < A.cull_alpha;
        if (A.toobig_on) {
            const bool big = size_now > A.cull_scale;                 // new rows carry max_2Dsize = 0
            tb_self = big || (A.screen_on && m2d > A.cull_screen);
            tb_kids = split && (big || (A.screen_on && 0.f > A.cull_screen));
            tb_dup = dup && (big || (A.screen_on && 0.f > A.cull_screen));
        }
        keep = !split && !alpha && !tb_self;
        kids = split && !alpha && !tb_kids;
        dup_keep = dup && !alpha && !tb_dup;
        flags[i] = (uint8_t)((keep ? F_KEEP : 0u) | (split ? F_SPLIT : 0u) | (kids ? F_KIDS : 0u) |
                             (dup_keep ? F_DUPKEEP : 0u) | (high ? F_HIGH : 0u) | (dup ? F_DUP : 0u));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c_keep = wave_count(keep), c_split = wave_count(split), c_kids = wave_count(kids);
    const int c_dupk = wave_count(dup_keep), c_high = wave_count(high), c_dup = wave_count(dup);
    const int c_big = wave_count(tb_self) + A.samps * wave_count(tb_kids) + wave_count(tb_dup);
    if (lane == 0) {
        int32_t *w = wsum[wave];
        w[0] = c_keep; w[1] = c_split; w[2] = c_kids; w[3] = c_dupk; w[4] = c_high; w[5] = c_dup; w[6] = c_big; w[7] = 0;
    }
    __syncthreads();
    if (threadIdx.x < DN_SUMS) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < DN_BLOCK / 64; ++w) s += wsum[w][threadIdx.x];
        blk[(size_t)blockIdx.x * DN_SUMS + threadIdx.x] = s;
    }
}

// One workgroup: blk[b][0..3] become the exclusive sums over the blocks before b; totals[0..7] the sums over all blocks
// (fixed order of integer additions).  Thread t owns the blocks [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void densify_scan_kernel(int nb, int32_t *__restrict__ blk,
                                                           int32_t *__restrict__ totals_ws,
                                                           int32_t *__restrict__ totals_out) {
    __shared__ int32_t part[256][DN_SUMS];
    const int per = (nb + 255) / 256;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    int32_t acc[DN_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = b0; b < b1; ++b)
#pragma unroll
        for (int k = 0; k < DN_SUMS; ++k) acc[k] += blk[(size_t)b * DN_SUMS + k];
#pragma unroll
    for (int k = 0; k < DN_SUMS; ++k) part[threadIdx.x][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < DN_SUMS) {             // exclusive scan of the 256 thread sums, one column per thread
        int32_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const int32_t v = part[t][threadIdx.x];
            part[t][threadIdx.x] = run;
            run += v;
        }
        totals_ws[threadIdx.x] = run;
        if (totals_out) totals_out[threadIdx.x] = run;
    }
    __syncthreads();
    int32_t run[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) run[k] = part[threadIdx.x][k];
    for (int b = b0; b < b1; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t v = blk[(size_t)b * DN_SUMS + k];
            blk[(size_t)b * DN_SUMS + k] = run[k];
            run[k] += v;
        }
}

// rank of this lane among the lanes of its workgroup that set `p`, through `scratch` (one int per wave)
__device__ __forceinline__ int block_rank(bool p, int32_t *scratch) {
    const unsigned long long m = __ballot(p);
    const int wave = threadIdx.x >> 6;
    const int in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if ((threadIdx.x & 63) == 0) scratch[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += scratch[w];
    return before + in_wave;
}

// The row map: src[r] = the input row that output row r derives from; kind[r] = 0 a copy, -1 a duplicate,
// 1 + noise row (= k * n_splits + rank among all split parents) child k of a split parent.
__global__ __launch_bounds__(DN_BLOCK) void densify_map_kernel(int n, int n_out, int samps,
                                                               const uint8_t *__restrict__ flags,
                                                               const int32_t *__restrict__ blk,
                                                               const int32_t *__restrict__ totals,
                                                               int32_t *__restrict__ src, int32_t *__restrict__ kind) {
    __shared__ int32_t scratch[4][DN_BLOCK / 64];
    const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
    const unsigned f = i < n ? flags[i] : 0u;
    const int32_t *off = blk + (size_t)blockIdx.x * DN_SUMS;
    const int r_keep = off[0] + block_rank(f & F_KEEP, scratch[0]);
    const int r_split = off[1] + block_rank(f & F_SPLIT, scratch[1]);
    const int r_kids = off[2] + block_rank(f & F_KIDS, scratch[2]);
    const int r_dup = off[3] + block_rank(f & F_DUPKEEP, scratch[3]);
    const int kept = totals[0], n_splits = totals[1], kept_parents = totals[2];
    if (f & F_KEEP) {
        if (r_keep < n_out) { src[r_keep] = i; kind[r_keep] = 0; }
    }
    if (f & F_KIDS) {
        for (int k = 0; k < samps; ++k) {       // sample-major, like .repeat(samps, 1)
            const int64_t r = (int64_t)kept + (int64_t)k * kept_parents + r_kids;
            if (r < n_out) { src[r] = i; kind[r] = 1 + k * n_splits + r_split; }
        }
    }
    if (f & F_DUPKEEP) {
        const int64_t r = (int64_t)kept + (int64_t)samps * kept_parents + r_dup;
        if (r < n_out) { src[r] = i; kind[r] = -1; }
    }
}

struct ApplyTable {
    const float *in[DN_MAX_TENSORS];
    float *out[DN_MAX_TENSORS];
    int row[DN_MAX_TENSORS];                // floats per row
    int role[DN_MAX_TENSORS];
    int blk_start[DN_MAX_TENSORS + 1];      // first workgroup of each tensor
    int count;
};

struct ApplyShared {
    int n, n_out;
    int64_t noise_rows;
    const int32_t *src, *kind;
    const uint8_t *flags;
    const float *means, *log_scales, *quats, *noise;
};

// component c of  R(q / |q|) (exp(log_scales) * noise) + mean  for input row s and noise row nr, in the order of the
// torch expressions (quat_to_rotmat normalises once more; no contraction)
__device__ __forceinline__ float child_mean(const ApplyShared &S, int s, int64_t nr, int c) {
    const float4 q4 = *reinterpret_cast<const float4 *>(S.quats + 4 * (size_t)s);
    const float n1 = sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
    float w = q4.x / n1, x = q4.y / n1, y = q4.z / n1, z = q4.w / n1;
    const float n2 = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-12f);
    w = w / n2; x = x / n2; y = y / n2; z = z / n2;
    float r0, r1, r2;
    if (c == 0) { r0 = 1.f - 2.f * (y * y + z * z); r1 = 2.f * (x * y - w * z); r2 = 2.f * (x * z + w * y); }
    else if (c == 1) { r0 = 2.f * (x * y + w * z); r1 = 1.f - 2.f * (x * x + z * z); r2 = 2.f * (y * z - w * x); }
    else { r0 = 2.f * (x * z - w * y); r1 = 2.f * (y * z + w * x); r2 = 1.f - 2.f * (x * x + y * y); }
    const float *ls = S.log_scales + 3 * (size_t)s, *nz = S.noise + 3 * (size_t)nr;
    const float s0 = expf(ls[0]) * nz[0], s1 = expf(ls[1]) * nz[1], s2 = expf(ls[2]) * nz[2];
    return (r0 * s0 + r1 * s1 + r2 * s2) + S.means[3 * (size_t)s + c];
}

__global__ __launch_bounds__(256) void densify_apply_kernel(ApplyTable T, ApplyShared S) {
    int t = 0;
    while (t + 1 < T.count && (int)blockIdx.x >= T.blk_start[t + 1]) ++t;
    const int rf = T.row[t], role = T.role[t];
    const float *__restrict__ in = T.in[t];
    float *__restrict__ out = T.out[t];
    const int64_t total = (int64_t)S.n_out * rf;
    const int64_t base = (int64_t)(blockIdx.x - T.blk_start[t]) * DN_CHUNK;
    const bool vec = (((uintptr_t)out) & 15) == 0;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int64_t e0 = base + ((int64_t)it * 256 + threadIdx.x) * 4;
        if (e0 >= total) break;
        int64_t r = e0 / rf;
        int c = (int)(e0 - r * rf);
        float v[4];
        int s = -1, k = 0;
        bool fresh = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j < total) {
                if (fresh) { s = S.src[r]; k = S.kind[r]; fresh = false; }
                float x = 0.f;
                if ((unsigned)s < (unsigned)S.n) {
                    const size_t at = (size_t)s * rf + c;
                    if (role == ROLE_MOMENT) x = k == 0 ? in[at] : 0.f;
                    else if (role == ROLE_COPY) x = in[at];
                    else if (role == ROLE_LOG_SCALES) {
                        x = in[at];
                        if (k > 0 || (k < 0 && (S.flags[s] & F_SPLIT))) x = shrink(x);
                    } else {
                        if (k > 0 && (int64_t)(k - 1) < S.noise_rows) x = child_mean(S, s, k - 1, c);
                        else x = in[at];
                    }
                }
                v[j] = x;
                if (++c == rf) { c = 0; ++r; fresh = true; }
            } else v[j] = 0.f;
        }
        if (vec && e0 + 4 <= total) *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int j = 0; j < 4 && e0 + j < total; ++j) out[e0 + j] = v[j];
    }
}

}  // namespace

SGN_EXPORT size_t sgn_densify_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return ws_flags_bytes(n) + ws_blk_bytes(n) + al256(DN_TOTALS * sizeof(int32_t));
}

SGN_EXPORT int sgn_densify_decide(int n, const float *xys_grad_norm, const float *vis_counts, const float *max_2dsize,
                                  const float *log_scales, const float *opacity_logits, float densify_grad_thresh,
                                  float densify_size_thresh, float split_screen_size, float cull_alpha_thresh,
                                  float cull_scale_thresh, float cull_screen_size, float image_dim,
                                  int n_split_samples, int densify, int screen_size_tests, int too_big_culls, void *ws,
                                  size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    SGN_ARG_CHECK(n_split_samples >= 1 && n_split_samples <= 64, -2);
    SGN_ARG_CHECK((int64_t)n * (n_split_samples + 2) <= (int64_t)INT32_MAX, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(log_scales && opacity_logits && ws, -3);
    SGN_ARG_CHECK(!densify || (xys_grad_norm && vis_counts), -3);
    SGN_ARG_CHECK(!screen_size_tests || max_2dsize, -3);
    SGN_ARG_CHECK(!densify || image_dim > 0.f, -4);
    SGN_ARG_CHECK(ws_bytes >= sgn_densify_workspace_bytes(n), -5);
    DecideArgs A;
    A.grad_thresh = densify_grad_thresh; A.size_thresh = densify_size_thresh; A.split_screen = split_screen_size;
    A.cull_alpha = cull_alpha_thresh; A.cull_scale = cull_scale_thresh; A.cull_screen = cull_screen_size;
    A.dim = image_dim; A.samps = n_split_samples; A.densify = densify != 0; A.screen_on = screen_size_tests != 0;
    A.toobig_on = too_big_culls != 0;
    uint8_t *flags = (uint8_t *)ws;
    int32_t *blk = (int32_t *)((char *)ws + ws_flags_bytes(n));
    hipLaunchKernelGGL(densify_decide_kernel, dim3(sgn_cdiv(n, DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)stream, n,
                       xys_grad_norm, vis_counts, max_2dsize, log_scales, opacity_logits, A, flags, blk);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_densify_scan(int n, void *ws, size_t ws_bytes, int32_t *totals8, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(ws && totals8, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_densify_workspace_bytes(n), -5);
    int32_t *blk = (int32_t *)((char *)ws + ws_flags_bytes(n));
    int32_t *totals_ws = (int32_t *)((char *)ws + ws_flags_bytes(n) + ws_blk_bytes(n));
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sgn_cdiv(n, DN_BLOCK), blk,
                       totals_ws, totals8);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_densify_apply(int n, int n_out, int n_split_samples, int64_t noise_rows, const float *means,
                                 const float *log_scales, const float *quats, const float *noise, int count,
                                 const float *const *inputs, float *const *outputs, const int32_t *row_floats,
                                 const int32_t *roles, int32_t *src, int32_t *kind, const void *ws, size_t ws_bytes,
                                 sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0 && n_out >= 0, -1);
    SGN_ARG_CHECK(n_split_samples >= 1 && n_split_samples <= 64, -2);
    SGN_ARG_CHECK((int64_t)n * (n_split_samples + 2) <= (int64_t)INT32_MAX && n_out <= n * (n_split_samples + 2), -1);
    SGN_ARG_CHECK(count >= 0 && count <= DN_MAX_TENSORS && noise_rows >= 0, -6);
    if (n == 0 || n_out == 0) return 0;
    SGN_ARG_CHECK(src && kind && ws, -3);
    SGN_ARG_CHECK(count == 0 || (inputs && outputs && row_floats && roles), -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_densify_workspace_bytes(n), -5);
    ApplyTable T;
    T.count = 0;
    int64_t blocks = 0;
    bool computed = false;
    for (int i = 0; i < count; ++i) {
        SGN_ARG_CHECK(inputs[i] && outputs[i] && inputs[i] != outputs[i], -3);
        SGN_ARG_CHECK(row_floats[i] >= 1 && roles[i] >= ROLE_COPY && roles[i] <= ROLE_MOMENT, -6);
        SGN_ARG_CHECK((roles[i] != ROLE_MEANS && roles[i] != ROLE_LOG_SCALES) || row_floats[i] == 3, -6);
        computed = computed || roles[i] == ROLE_MEANS;
        const int k = T.count++;
        T.in[k] = inputs[i]; T.out[k] = outputs[i]; T.row[k] = row_floats[i]; T.role[k] = roles[i];
        T.blk_start[k] = (int)blocks;
        blocks += ((int64_t)n_out * row_floats[i] + DN_CHUNK - 1) / DN_CHUNK;
        SGN_ARG_CHECK(blocks <= (int64_t)INT32_MAX, -6);
    }
    T.blk_start[T.count] = (int)blocks;
    SGN_ARG_CHECK(!computed || noise_rows == 0 || (means && log_scales && quats && noise), -3);
    SGN_ARG_CHECK(!computed || (((uintptr_t)quats) & 15) == 0, -7);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *flags = (const uint8_t *)ws;
    const int32_t *blk = (const int32_t *)((const char *)ws + ws_flags_bytes(n));
    const int32_t *totals = (const int32_t *)((const char *)ws + ws_flags_bytes(n) + ws_blk_bytes(n));
    hipLaunchKernelGGL(densify_map_kernel, dim3(sgn_cdiv(n, DN_BLOCK)), dim3(DN_BLOCK), 0, s, n, n_out, n_split_samples,
                       flags, blk, totals, src, kind);
    if (blocks > 0) {
        ApplyShared S;
        S.n = n; S.n_out = n_out; S.noise_rows = noise_rows; S.src = src; S.kind = kind; S.flags = flags;
        S.means = means; S.log_scales = log_scales; S.quats = quats; S.noise = noise;
        hipLaunchKernelGGL(densify_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T, S);
    }
    SGN_LAUNCH_CHECK();
    return 0;
}
