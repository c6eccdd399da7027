// mcmc.hip — fixed-budget MCMC refinement ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy)
// as HIP passes, gfx950: hashed relocation of dead Gaussians onto live ones, growth up to a cap, per-step noise.
// Decided here from the published algorithm, unpinned; sgn_rast.mcmc's torch engine restates every line.
//
// THE ARITHMETIC CONTRACT (both engines and tests/mcmc_oracle.py follow it).
//   mix64 = densify._mix64 (the splitmix64 finaliser).  key_p = mix64(seed * 1000003 + step + (p << 56)) on the host,
//   p = 1 relocate, 2 grow, 3 noise.
//   weights  o = 1 / (1 + exp(-(double)logit));  dead = o <= (double)(float)min_opacity;
//            w = (int64)floor(o * 2^24 + 0.5) (0 for a NaN);  relocate: a dead row has w = 0, grow: every row keeps w;
//            P = exclusive int64 prefix of w, total = its sum (integers: exact in any order).
//   draws    h_j = mix64(mix64(j + 1) ^ key_p);  t_j = (h_j >>> 1) mod total;  s_j = the row with P[s] <= t_j < P[s] + w[s].
//            relocate: K = n_dead, target d_j = the j-th dead row in row order;  grow: targets are the new rows N + j.
//   ratios   N_j = min(n_max, 1 + c[s_j]),  c[s] = the number of this phase's draws that chose s (integer atomics).
//   values   in fp64 from the fp32 inputs, rounded to fp32 once, no contraction:
//            x = 1 - pow(1 - o, 1 / N);   S = sum_{i=1..N} inner_i,  inner_i = sum_{k=0..i-1} term_ik (k ascending),
//            term_ik = ((C(i-1,k) (-1)^k) * x^(k+1)) * (1 / sqrt(k+1)),  x^(k+1) by repeated multiplication from x;
//            x' = min(max(x, (double)(float)min_opacity), 1 - 2^-23);  logit' = (float)log(x' / (1 - x'));
//            log_scale_c' = (float)((double)log_scale_c + log(o / S)).
//            (fp64 on purpose: in fp32 the alternating sum cancels about six digits, o / S is off by 1.4e-3 at N = 51.)
//   writes   relocate, in place: all parameters of row d_j = row s_j's with the new logit / log-scales; row s_j gets the
//            new logit / log-scales and zeroed moments; d_j's moments keep their bits; nothing else changes a bit.
//            grow, old -> new: rows < N copy (sources get the new values, moments unchanged), row N + j copies s_j with
//            the new values, zero moments.  Draws that share a source write identical values.
//   noise    b = mix64(mix64(row + 1) ^ key_3);  u_m = ((double)(mix64(b + m) >>> 11) + 0.5) * 2^-53, m = 1..4;
//            r1 = sqrt(-2 ln u1), r2 = sqrt(-2 ln u3);  z = (r1 cos(2 pi u2), r1 sin(2 pi u2), r2 cos(2 pi u4)) in fp64,
//            rounded to fp32.  Then fp32: g = 1 / (1 + exp(-100 ((1 - sigmoid(logit)) - 0.995)));
//            Sigma = R diag(exp(log_scales))^2 R^T, R from q / |q| by gsplat's quat_to_rotmat;
//            means += Sigma ((z * g) * scaler).
// The binomials (51 x 51 doubles, exact integers) live in constant memory; the 51 reciprocal roots are formed on the
// host with IEEE sqrt and division and travel as a kernel argument, so every engine holds the same doubles.
#include <math.h>

#include "sgn_common.h"

namespace {

constexpr int MC_BLOCK = 256;
constexpr int MC_NMAX = 51;
constexpr int MC_MAX_TENSORS = 24;

enum { ROLE_COPY = 0, ROLE_LOGIT = 1, ROLE_LOG_SCALES = 2, ROLE_MOMENT = 3 };
enum { MODE_RELOCATE = 0, MODE_GROW = 1 };

struct Binomials { double c[MC_NMAX][MC_NMAX]; };
constexpr Binomials pascal() {
    Binomials b{};
    for (int m = 0; m < MC_NMAX; ++m)
        for (int k = 0; k <= m; ++k) b.c[m][k] = (k == 0 || k == m) ? 1.0 : b.c[m - 1][k - 1] + b.c[m - 1][k];
    return b;
}
__constant__ Binomials BINOM = pascal();
struct InvSqrt { double r[MC_NMAX]; };

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x *= 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int n_blocks(int n) { return sgn_cdiv(n, MC_BLOCK); }

// workspace: per-block sums of the weights (int64) and of the dead flags (int32), the totals, and two per-row words:
// the draw count c[s] and the largest draw index that chose s
struct Ws {
    int64_t *blk_w, *totals;
    int32_t *blk_dead, *count, *owner;
};
inline size_t ws_bytes_for(int n) {
    const size_t nb = (size_t)n_blocks(n);
    return al256(nb * sizeof(int64_t)) + al256(nb * sizeof(int32_t)) + al256(2 * sizeof(int64_t)) +
           2 * al256((size_t)n * sizeof(int32_t));
}
inline Ws carve(void *ws, int n) {
    const size_t nb = (size_t)n_blocks(n);
    char *p = (char *)ws;
    Ws W;
    W.blk_w = (int64_t *)p; p += al256(nb * sizeof(int64_t));
    W.blk_dead = (int32_t *)p; p += al256(nb * sizeof(int32_t));
    W.totals = (int64_t *)p; p += al256(2 * sizeof(int64_t));
    W.count = (int32_t *)p; p += al256((size_t)n * sizeof(int32_t));
    W.owner = (int32_t *)p;
    return W;
}

__global__ __launch_bounds__(MC_BLOCK) void mcmc_weights_kernel(int n, const float *__restrict__ logits,
                                                                float min_opacity, int relocate,
                                                                int32_t *__restrict__ w, uint8_t *__restrict__ dead,
                                                                int64_t *__restrict__ blk_w,
                                                                int32_t *__restrict__ blk_dead) {
    __shared__ int32_t ws_w[MC_BLOCK / 64], ws_d[MC_BLOCK / 64];
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    int32_t wi = 0;
    bool d = false;
    if (i < n) {
        const double o = 1.0 / (1.0 + exp(-(double)logits[i]));
        d = o <= (double)min_opacity;
        wi = (o == o) ? (int32_t)floor(o * 16777216.0 + 0.5) : 0;
        if (relocate && d) wi = 0;
        w[i] = wi;
        dead[i] = d ? 1 : 0;
    }
    int32_t s = wi;                                     // a wave's sum is at most 64 * 2^24
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    const int nd = __popcll(__ballot(d));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ws_w[wave] = s; ws_d[wave] = nd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t tw = 0;
        int32_t td = 0;
#pragma unroll
        for (int k = 0; k < MC_BLOCK / 64; ++k) { tw += ws_w[k]; td += ws_d[k]; }
        blk_w[blockIdx.x] = tw;
        blk_dead[blockIdx.x] = td;
    }
}

// One workgroup: the block sums become exclusive offsets; totals = [n_dead, total].  Thread t owns the blocks
// [t * per, (t + 1) * per): the second level of the scan for more than 256 blocks.
__global__ __launch_bounds__(256) void mcmc_scan_blocks_kernel(int nb, int64_t *__restrict__ blk_w,
                                                               int32_t *__restrict__ blk_dead,
                                                               int64_t *__restrict__ totals_ws,
                                                               int64_t *__restrict__ totals_out) {
    __shared__ int64_t part_w[256];
    __shared__ int32_t part_d[256];
    const int per = (nb + 255) / 256;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    int64_t aw = 0;
    int32_t ad = 0;
    for (int b = b0; b < b1; ++b) { aw += blk_w[b]; ad += blk_dead[b]; }
    part_w[threadIdx.x] = aw;
    part_d[threadIdx.x] = ad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t rw = 0;
        int32_t rd = 0;
        for (int t = 0; t < 256; ++t) {
            const int64_t vw = part_w[t];
            const int32_t vd = part_d[t];
            part_w[t] = rw; part_d[t] = rd;
            rw += vw; rd += vd;
        }
        totals_ws[0] = rd; totals_ws[1] = rw;
        totals_out[0] = rd; totals_out[1] = rw;
    }
    __syncthreads();
    int64_t rw = part_w[threadIdx.x];
    int32_t rd = part_d[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        const int64_t vw = blk_w[b];
        const int32_t vd = blk_dead[b];
        blk_w[b] = rw; blk_dead[b] = rd;
        rw += vw; rd += vd;
    }
}

// Per row: the exclusive prefix of the weights, and the row's place among the dead rows.
__global__ __launch_bounds__(MC_BLOCK) void mcmc_scan_rows_kernel(int n, const int32_t *__restrict__ w,
                                                                  const uint8_t *__restrict__ dead,
                                                                  const int64_t *__restrict__ blk_w,
                                                                  const int32_t *__restrict__ blk_dead,
                                                                  int64_t *__restrict__ prefix,
                                                                  int32_t *__restrict__ dead_rows) {
    __shared__ int32_t wave_w[MC_BLOCK / 64], wave_d[MC_BLOCK / 64];
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t wi = i < n ? w[i] : 0;
    const bool d = i < n && dead[i] != 0;
    int32_t inc = wi;                                   // inclusive scan inside the wave (at most 64 * 2^24)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    const unsigned long long m = __ballot(d);
    const int d_before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 63) wave_w[wave] = inc;
    if (lane == 0) wave_d[wave] = __popcll(m);
    __syncthreads();
    int64_t before_w = blk_w[blockIdx.x];
    int32_t before_d = blk_dead[blockIdx.x];
    for (int k = 0; k < wave; ++k) { before_w += wave_w[k]; before_d += wave_d[k]; }
    if (i < n) {
        prefix[i] = before_w + (int64_t)(inc - wi);
        if (d) {
            const int at = before_d + d_before;
            if (at < n) dead_rows[at] = i;
        }
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mcmc_draw_kernel(int n, int k, uint64_t key,
                                                             const int64_t *__restrict__ prefix,
                                                             const int64_t *__restrict__ totals,
                                                             int32_t *__restrict__ src, int32_t *__restrict__ count) {
    const int j = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (j >= k) return;
    const int64_t total = totals[1];
    int s = 0;
    if (total > 0) {
        const uint64_t h = mix64(mix64((uint64_t)j + 1ull) ^ key);
        const int64_t t = (int64_t)((h >> 1) % (uint64_t)total);
        int lo = 0, hi = n;                             // the first row whose prefix exceeds t; its predecessor owns t
        while (lo < hi) {
            const int mid = (int)(((int64_t)lo + hi) >> 1);
            if (prefix[mid] <= t) lo = mid + 1; else hi = mid;
        }
        s = max(lo - 1, 0);
    }
    src[j] = s;
    atomicAdd(&count[s], 1);
}

__global__ __launch_bounds__(MC_BLOCK) void mcmc_ratio_kernel(int n, int k, int n_max, const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ count,
                                                              int32_t *__restrict__ ratio, int32_t *__restrict__ owner) {
    const int j = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (j >= k) return;
    const int s = src[j];
    if ((unsigned)s >= (unsigned)n) { ratio[j] = 1; return; }
    ratio[j] = min(n_max, 1 + count[s]);
    atomicMax(&owner[s], j);
}

__global__ __launch_bounds__(MC_BLOCK) void mcmc_relocation_kernel(int n, int k, const float *__restrict__ logits,
                                                                   const float *__restrict__ log_scales,
                                                                   float min_opacity, const int32_t *__restrict__ src,
                                                                   const int32_t *__restrict__ ratio, InvSqrt R,
                                                                   float *__restrict__ staging) {
    const int j = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (j >= k) return;
    const int s = src[j];
    if ((unsigned)s >= (unsigned)n) return;
    const int N = min(max(ratio[j], 1), MC_NMAX);
    const double o = 1.0 / (1.0 + exp(-(double)logits[s]));
    const double x = 1.0 - pow(1.0 - o, 1.0 / (double)N);
    double S = 0.0;
    for (int i = 1; i <= N; ++i) {
        double inner = 0.0, p = x;
        for (int q = 0; q < i; ++q) {
            const double b = (q & 1) ? -BINOM.c[i - 1][q] : BINOM.c[i - 1][q];
            inner += (b * p) * R.r[q];
            p *= x;
        }
        S += inner;
    }
    const double xc = fmin(fmax(x, (double)min_opacity), 1.0 - 0x1p-23);
    const double shift = log(o / S);
    float *out = staging + 4 * (size_t)j;
    out[0] = (float)log(xc / (1.0 - xc));
#pragma unroll
    for (int c = 0; c < 3; ++c) out[1 + c] = (float)((double)log_scales[3 * (size_t)s + c] + shift);
}

struct ApplyTable {
    const float *in[MC_MAX_TENSORS];
    float *out[MC_MAX_TENSORS];
    int row[MC_MAX_TENSORS];                // floats per row
    int role[MC_MAX_TENSORS];
    int blk_start[MC_MAX_TENSORS + 1];      // first workgroup of each tensor
    int count;
};

// One lane per (draw, element) in place for relocate, per output element for grow.  Relocate reads source rows of the
// copied parameters only (live rows: never a target) and takes every computed value from `staging`.
__global__ __launch_bounds__(MC_BLOCK) void mcmc_apply_kernel(ApplyTable T, int mode, int n, int k,
                                                              const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ targets,
                                                              const int32_t *__restrict__ owner,
                                                              const float *__restrict__ staging) {
    int t = 0;
    while (t + 1 < T.count && (int)blockIdx.x >= T.blk_start[t + 1]) ++t;
    const int rf = T.row[t], role = T.role[t];
    const float *in = T.in[t];
    float *out = T.out[t];
    const int64_t rows = mode == MODE_RELOCATE ? (int64_t)k : (int64_t)n + k;
    const int64_t e = (int64_t)(blockIdx.x - T.blk_start[t]) * MC_BLOCK + threadIdx.x;
    if (e >= rows * rf) return;
    const int64_t r = e / rf;
    const int c = (int)(e - r * rf);
    if (mode == MODE_RELOCATE) {
        const int s = src[r], d = targets[r];
        if ((unsigned)s >= (unsigned)n || (unsigned)d >= (unsigned)n) return;
        if (role == ROLE_MOMENT) { out[(size_t)s * rf + c] = 0.f; return; }
        if (role == ROLE_COPY) { out[(size_t)d * rf + c] = in[(size_t)s * rf + c]; return; }
        const float v = staging[4 * (size_t)r + (role == ROLE_LOGIT ? 0 : 1 + c)];
        out[(size_t)d * rf + c] = v;
        out[(size_t)s * rf + c] = v;
        return;
    }
    int s, j;
    if (r < n) { s = (int)r; j = owner[r]; }
    else { j = (int)(r - n); s = src[j]; }
    float v = 0.f;
    if ((unsigned)s < (unsigned)n) {
        if (role == ROLE_MOMENT) v = r < n ? in[(size_t)s * rf + c] : 0.f;
        else if (role == ROLE_COPY || j < 0 || j >= k) v = in[(size_t)s * rf + c];
        else v = staging[4 * (size_t)j + (role == ROLE_LOGIT ? 0 : 1 + c)];
    }
    out[e] = v;
}

// The per-step stream: 44 bytes read and 12 written per row, no LDS, no atomics.
__global__ __launch_bounds__(MC_BLOCK) void mcmc_noise_kernel(int n, uint64_t key, float scaler,
                                                              float *__restrict__ means,
                                                              const float *__restrict__ log_scales,
                                                              const float *__restrict__ quats,
                                                              const float *__restrict__ logits,
                                                              float *__restrict__ z_out) {
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 q4 = *reinterpret_cast<const float4 *>(quats + 4 * (size_t)i);
    const float l0 = log_scales[3 * (size_t)i], l1 = log_scales[3 * (size_t)i + 1], l2 = log_scales[3 * (size_t)i + 2];
    const float logit = logits[i];
    float *mp = means + 3 * (size_t)i;
    const float m0 = mp[0], m1 = mp[1], m2 = mp[2];

    const uint64_t b = mix64(mix64((uint64_t)i + 1ull) ^ key);
    double u[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) u[m] = ((double)(mix64(b + (uint64_t)(m + 1)) >> 11) + 0.5) * 0x1p-53;
    const double two_pi = 2.0 * 3.14159265358979323846;
    const double r1 = sqrt(-2.0 * log(u[0])), r2 = sqrt(-2.0 * log(u[2]));
    const double a1 = two_pi * u[1], a2 = two_pi * u[3];
    const float z0 = (float)(r1 * cos(a1)), z1 = (float)(r1 * sin(a1)), z2 = (float)(r2 * cos(a2));
    if (z_out) { z_out[3 * (size_t)i] = z0; z_out[3 * (size_t)i + 1] = z1; z_out[3 * (size_t)i + 2] = z2; }

    const float sig = 1.f / (1.f + expf(-logit));
    const float g = 1.f / (1.f + expf(-100.f * ((1.f - sig) - 0.995f)));
    const float v0 = (z0 * g) * scaler, v1 = (z1 * g) * scaler, v2 = (z2 * g) * scaler;

    const float n1 = sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
    float w = q4.x / n1, x = q4.y / n1, y = q4.z / n1, z = q4.w / n1;
    const float n2 = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-12f);
    w = w / n2; x = x / n2; y = y / n2; z = z / n2;
    const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - w * z), r02 = 2.f * (x * z + w * y);
    const float r10 = 2.f * (x * y + w * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - w * x);
    const float r20 = 2.f * (x * z - w * y), r21 = 2.f * (y * z + w * x), r22 = 1.f - 2.f * (x * x + y * y);
    const float s0 = expf(l0), s1 = expf(l1), s2 = expf(l2);
    // Sigma v = R (s^2 * (R^T v))
    const float y0 = (s0 * s0) * (r00 * v0 + r10 * v1 + r20 * v2);
    const float y1 = (s1 * s1) * (r01 * v0 + r11 * v1 + r21 * v2);
    const float y2 = (s2 * s2) * (r02 * v0 + r12 * v1 + r22 * v2);
    mp[0] = m0 + (r00 * y0 + r01 * y1 + r02 * y2);
    mp[1] = m1 + (r10 * y0 + r11 * y1 + r12 * y2);
    mp[2] = m2 + (r20 * y0 + r21 * y1 + r22 * y2);
}

}  // namespace

SGN_EXPORT size_t sgn_mcmc_workspace_bytes(int n) { return n <= 0 ? 0 : ws_bytes_for(n); }

SGN_EXPORT int sgn_mcmc_weights(int n, const float *opacity_logits, float min_opacity, int relocate, int32_t *w,
                                uint8_t *dead, void *ws, size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(opacity_logits && w && dead && ws, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_mcmc_workspace_bytes(n), -5);
    const Ws W = carve(ws, n);
    hipLaunchKernelGGL(mcmc_weights_kernel, dim3(n_blocks(n)), dim3(MC_BLOCK), 0, (hipStream_t)stream, n, opacity_logits,
                       min_opacity, relocate != 0, w, dead, W.blk_w, W.blk_dead);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_mcmc_scan(int n, const int32_t *w, const uint8_t *dead, int64_t *prefix, int32_t *dead_rows,
                             void *ws, size_t ws_bytes, int64_t *totals2, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(w && dead && prefix && dead_rows && ws && totals2, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_mcmc_workspace_bytes(n), -5);
    const Ws W = carve(ws, n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mcmc_scan_blocks_kernel, dim3(1), dim3(256), 0, s, n_blocks(n), W.blk_w, W.blk_dead, W.totals,
                       totals2);
    hipLaunchKernelGGL(mcmc_scan_rows_kernel, dim3(n_blocks(n)), dim3(MC_BLOCK), 0, s, n, w, dead, W.blk_w, W.blk_dead,
                       prefix, dead_rows);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_mcmc_draw(int n, int k, int64_t key, int n_max, const int64_t *prefix, int32_t *src, int32_t *ratio,
                             void *ws, size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0 && k >= 0, -1);
    SGN_ARG_CHECK((int64_t)n + (int64_t)k <= (int64_t)INT32_MAX, -1);
    SGN_ARG_CHECK(n_max >= 1 && n_max <= MC_NMAX, -2);
    if (n == 0 || k == 0) return 0;
    SGN_ARG_CHECK(prefix && src && ratio && ws, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_mcmc_workspace_bytes(n), -5);
    const Ws W = carve(ws, n);
    hipStream_t s = (hipStream_t)stream;
    SGN_HIP_CHECK(hipMemsetAsync(W.count, 0, (size_t)n * sizeof(int32_t), s));
    SGN_HIP_CHECK(hipMemsetAsync(W.owner, 0xFF, (size_t)n * sizeof(int32_t), s));
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(n_blocks(k)), dim3(MC_BLOCK), 0, s, n, k, (uint64_t)key, prefix, W.totals,
                       src, W.count);
    hipLaunchKernelGGL(mcmc_ratio_kernel, dim3(n_blocks(k)), dim3(MC_BLOCK), 0, s, n, k, n_max, src, W.count, ratio,
                       W.owner);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_mcmc_relocation(int n, int k, const float *opacity_logits, const float *log_scales, float min_opacity,
                                   const int32_t *src, const int32_t *ratio, float *staging, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0 && k >= 0, -1);
    if (n == 0 || k == 0) return 0;
    SGN_ARG_CHECK(opacity_logits && log_scales && src && ratio && staging, -3);
    InvSqrt R;
    for (int q = 0; q < MC_NMAX; ++q) R.r[q] = 1.0 / sqrt((double)(q + 1));
    hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(n_blocks(k)), dim3(MC_BLOCK), 0, (hipStream_t)stream, n, k,
                       opacity_logits, log_scales, min_opacity, src, ratio, R, staging);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_mcmc_apply(int mode, int n, int k, const int32_t *src, const int32_t *targets, const float *staging,
                              int count, const float *const *inputs, float *const *outputs, const int32_t *row_floats,
                              const int32_t *roles, const void *ws, size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(mode == MODE_RELOCATE || mode == MODE_GROW, -4);
    SGN_ARG_CHECK(n >= 0 && k >= 0, -1);
    SGN_ARG_CHECK((int64_t)n + (int64_t)k <= (int64_t)INT32_MAX, -1);
    SGN_ARG_CHECK(mode != MODE_RELOCATE || k <= n, -1);
    SGN_ARG_CHECK(count >= 0 && count <= MC_MAX_TENSORS, -6);
    if (n == 0 || k == 0 || count == 0) return 0;
    SGN_ARG_CHECK(src && staging && ws, -3);
    SGN_ARG_CHECK(mode != MODE_RELOCATE || targets, -3);
    SGN_ARG_CHECK(inputs && outputs && row_floats && roles, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_mcmc_workspace_bytes(n), -5);
    const int64_t rows = mode == MODE_RELOCATE ? (int64_t)k : (int64_t)n + k;
    ApplyTable T;
    T.count = 0;
    int64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        SGN_ARG_CHECK(inputs[i] && outputs[i], -3);
        SGN_ARG_CHECK(mode == MODE_RELOCATE ? inputs[i] == outputs[i] : inputs[i] != outputs[i], -3);
        SGN_ARG_CHECK(row_floats[i] >= 1 && roles[i] >= ROLE_COPY && roles[i] <= ROLE_MOMENT, -6);
        SGN_ARG_CHECK(roles[i] != ROLE_LOGIT || row_floats[i] == 1, -6);
        SGN_ARG_CHECK(roles[i] != ROLE_LOG_SCALES || row_floats[i] == 3, -6);
        const int q = T.count++;
        T.in[q] = inputs[i]; T.out[q] = outputs[i]; T.row[q] = row_floats[i]; T.role[q] = roles[i];
        T.blk_start[q] = (int)blocks;
        blocks += (rows * row_floats[i] + MC_BLOCK - 1) / MC_BLOCK;
        SGN_ARG_CHECK(blocks <= (int64_t)INT32_MAX, -6);
    }
    T.blk_start[T.count] = (int)blocks;
    const Ws W = carve(const_cast<void *>(ws), n);
    hipLaunchKernelGGL(mcmc_apply_kernel, dim3((unsigned)blocks), dim3(MC_BLOCK), 0, (hipStream_t)stream, T, mode, n, k,
                       src, targets, W.owner, staging);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_mcmc_noise(int n, int64_t key, float scaler, float *means, const float *log_scales,
                              const float *quats, const float *opacity_logits, float *z_out, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(means && log_scales && quats && opacity_logits, -3);
    SGN_ARG_CHECK((((uintptr_t)quats) & 15) == 0, -7);
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(n_blocks(n)), dim3(MC_BLOCK), 0, (hipStream_t)stream, n, (uint64_t)key,
                       scaler, means, log_scales, quats, opacity_logits, z_out);
    SGN_LAUNCH_CHECK();
    return 0;
}
