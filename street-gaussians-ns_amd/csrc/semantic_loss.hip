// semantic_loss.hip — softmax cross-entropy of a rendered logit image against a uint8 label map, gfx950.
//
// The semantic term of the Street Gaussians paper on the image that sgn_raster_features_fwd composites from
// per-Gaussian class logits: loss = mean over COUNTED pixels of (logsumexp(logits) - logits[label]), a pixel counting
// when its label differs from ignore_index, is a class (< K) and its mask byte (if a mask is given) is non-zero.  One
// thread per pixel (K <= 64: a pixel's logits are read from global memory once per pass, three passes in the forward,
// all served by the cache after the first).  The loss sum and the count are reduced on the device: per wave with
// shuffles — the sum in fp64, so that the mean carries the rounding of the per-pixel fp32 terms only — then one fp64
// and one integer atomic per wave; a one-thread launch forms the mean.  No host read-back: the backward reads the
// count and the incoming gradient from device memory.
#include "sgn_common.h"

namespace {

struct CeSums {
    double sum;            // sum of the counted pixels' losses
    unsigned int count;    // counted pixels
    unsigned int pad;
};
static_assert(sizeof(CeSums) == 16, "workspace layout");

__device__ __forceinline__ bool ce_counted(int p, int K, const unsigned char *__restrict__ labels, int ignore_index,
                                           const unsigned char *__restrict__ mask, int &label) {
    label = (int)labels[p];
    return label != ignore_index && label < K && (mask == nullptr || mask[p] != 0);
}

// max and sum of exp(l - max) of one pixel's logits.  The sum is formed in fp64: sixty-four fp32 additions would put
// several ulp into every softmax value of the pixel, more than the exp itself.
__device__ __forceinline__ void ce_softmax_terms(const float *__restrict__ row, int K, float &m, double &S) {
    m = row[0];
    for (int c = 1; c < K; ++c) m = fmaxf(m, row[c]);
    S = 0.0;
    for (int c = 0; c < K; ++c) S += (double)expf(row[c] - m);
}

__global__ __launch_bounds__(256) void ce_fwd_kernel(int n_pix, int K, const float *__restrict__ logits,
                                                     const unsigned char *__restrict__ labels, int ignore_index,
                                                     const unsigned char *__restrict__ mask, CeSums *__restrict__ sums) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    double loss = 0.0;
    unsigned int counted = 0u;
    if (p < n_pix) {
        int label;
        if (ce_counted(p, K, labels, ignore_index, mask, label)) {
            const float *row = logits + (size_t)p * (size_t)K;
            float m;
            double S;
            ce_softmax_terms(row, K, m, S);
            loss = (double)(m - row[label]) + (double)logf((float)S);
            counted = 1u;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        loss += __shfl_xor(loss, d, 64);
        counted += __shfl_xor(counted, d, 64);
    }
    if ((threadIdx.x & 63) == 0 && counted != 0u) {
        atomicAdd(&sums->sum, loss);
        atomicAdd(&sums->count, counted);
    }
}

__global__ void ce_mean_kernel(const CeSums *__restrict__ sums, float *__restrict__ loss_out) {
    // an image with no counted pixel: loss 0 (and, in the backward, zero gradient), not 0 / 0
    loss_out[0] = sums->count != 0u ? (float)(sums->sum / (double)sums->count) : 0.f;
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(int n_pix, int K, const float *__restrict__ logits,
                                                     const unsigned char *__restrict__ labels, int ignore_index,
                                                     const unsigned char *__restrict__ mask,
                                                     const float *__restrict__ v_loss,
                                                     const CeSums *__restrict__ sums, float *__restrict__ v_logits) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    float *out = v_logits + (size_t)p * (size_t)K;
    int label;
    if (!ce_counted(p, K, labels, ignore_index, mask, label)) {
        for (int c = 0; c < K; ++c) out[c] = 0.f;
        return;
    }
    const float *row = logits + (size_t)p * (size_t)K;
    float m;
    double S;
    ce_softmax_terms(row, K, m, S);
    // (softmax - onehot) * v_loss / count in fp64 from the fp32 exponentials: one rounding at the end
    const double inv = 1.0 / S, scale = (double)v_loss[0] / (double)sums->count;    // counted: the count is at least 1
    for (int c = 0; c < K; ++c) {
        const double sm = (double)expf(row[c] - m) * inv;
        out[c] = (float)((sm - (c == label ? 1.0 : 0.0)) * scale);
    }
}

int ce_check(const char *fn, int img_h, int img_w, int n_classes, int ignore_index) {
    if (!(img_h > 0 && img_w > 0 && (int64_t)img_h * img_w < ((int64_t)1 << 31))) {
        sgn_set_error("%s: argument check failed: 0 < img_h * img_w < 2^31", fn);
        return -1;
    }
    if (!(n_classes >= 1 && n_classes <= 64)) {
        sgn_set_error("%s: argument check failed: 1 <= n_classes <= 64", fn);
        return -2;
    }
    if (!(ignore_index >= -1 && ignore_index <= 255)) {
        sgn_set_error("%s: argument check failed: -1 <= ignore_index <= 255", fn);
        return -3;
    }
    return 0;
}

}  // namespace

SGN_EXPORT size_t sgn_semantic_ce_workspace_bytes(void) { return sizeof(CeSums); }

SGN_EXPORT int sgn_semantic_ce_fwd(int img_h, int img_w, int n_classes, const float *logits, const unsigned char *labels,
                                   int ignore_index, const unsigned char *mask, float *loss_out, void *ws,
                                   size_t ws_bytes, sgn_stream_t stream) {
    const int rc = ce_check(__func__, img_h, img_w, n_classes, ignore_index);
    if (rc != 0) return rc;
    SGN_ARG_CHECK(logits && labels && loss_out && ws, -4);
    SGN_ARG_CHECK(ws_bytes >= sizeof(CeSums), -5);
    hipStream_t s = (hipStream_t)stream;
    const int n_pix = img_h * img_w;
    SGN_HIP_CHECK(hipMemsetAsync(ws, 0, sizeof(CeSums), s));
    sgn_timing_begin(SGN_T_LOSS_FWD, s);
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(sgn_cdiv(n_pix, 256)), dim3(256), 0, s, n_pix, n_classes, logits, labels,
                       ignore_index, mask, (CeSums *)ws);
    hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(1), 0, s, (const CeSums *)ws, loss_out);
    sgn_timing_end(SGN_T_LOSS_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_semantic_ce_bwd(int img_h, int img_w, int n_classes, const float *logits, const unsigned char *labels,
                                   int ignore_index, const unsigned char *mask, const float *v_loss, const void *ws,
                                   size_t ws_bytes, float *v_logits, sgn_stream_t stream) {
    const int rc = ce_check(__func__, img_h, img_w, n_classes, ignore_index);
    if (rc != 0) return rc;
    SGN_ARG_CHECK(logits && labels && v_loss && ws && v_logits, -4);
    SGN_ARG_CHECK(ws_bytes >= sizeof(CeSums), -5);
    hipStream_t s = (hipStream_t)stream;
    const int n_pix = img_h * img_w;
    sgn_timing_begin(SGN_T_LOSS_BWD, s);
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(sgn_cdiv(n_pix, 256)), dim3(256), 0, s, n_pix, n_classes, logits, labels,
                       ignore_index, mask, v_loss, (const CeSums *)ws, v_logits);
    sgn_timing_end(SGN_T_LOSS_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}
