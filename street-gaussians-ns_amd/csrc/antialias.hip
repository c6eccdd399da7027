// antialias.hip — the antialiased rasterize mode's opacity compensation, gfx950.
//
// The reference's config has rasterize_mode "classic" | "antialiased" (sgn_splatfacto.py:214-222) and leaves the second
// dead: the projection's compensation factor is dropped (:860) and the multiply is commented out (:947,
// `torch.sigmoid(opacities) #* comp[:, None]`).  This pair makes it real for the fused surface, whose sigmoid otherwise
// lives inside the rasterizer's row build: the effective opacity o = sigmoid(logit) * compensation is formed ONCE per
// render and handed to every pass downstream as a probability (opacity_is_logit = 0), and its backward splits the
// passes' summed v_o into the logit's gradient and the factor's, which the projection backward takes as
// v_compensation.
// Pure streaming: one row per lane, 4-byte coalesced accesses (n is arbitrary and the tensors may be 4-byte-aligned
// slices of an arena), no LDS, no atomics; 12 bytes per row forward, at most 20 backward.
// The arithmetic is a contract (include/sgn_rast.h "ANTIALIASED OPACITY"): fp32, no contraction, the sigmoid spelled as
// the rasterizer's row build spells it (raster.hip), the chain evaluated left to right as its unpack does.
#include "sgn_common.h"

namespace {

__global__ __launch_bounds__(256) void aa_opacity_fwd_kernel(int n, const float *__restrict__ logits,
                                                             const float *__restrict__ comp,
                                                             float *__restrict__ opac) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = 1.f / (1.f + expf(-logits[i]));
    opac[i] = s * comp[i];
}

// v_logits / v_comp: either may be NULL (not wanted)
__global__ __launch_bounds__(256) void aa_opacity_bwd_kernel(int n, const float *__restrict__ logits,
                                                             const float *__restrict__ comp,
                                                             const float *__restrict__ v_opac,
                                                             float *__restrict__ v_logits,
                                                             float *__restrict__ v_comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = 1.f / (1.f + expf(-logits[i]));
    const float vo = v_opac[i];
    if (v_logits != nullptr) {
        float v = vo * comp[i];
        v = v * s * (1.f - s);
        v_logits[i] = v;
    }
    if (v_comp != nullptr) v_comp[i] = vo * s;
}

}  // namespace

SGN_EXPORT int sgn_aa_opacity_fwd(int n, const float *opacity_logits, const float *compensation, float *opacities,
                                  sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(opacity_logits && compensation && opacities, -2);
    hipLaunchKernelGGL(aa_opacity_fwd_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n,
                       opacity_logits, compensation, opacities);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_aa_opacity_bwd(int n, const float *opacity_logits, const float *compensation,
                                  const float *v_opacities, float *v_opacity_logits, float *v_compensation,
                                  sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    if (n == 0) return 0;
    SGN_ARG_CHECK(opacity_logits && compensation && v_opacities, -2);
    if (v_opacity_logits == nullptr && v_compensation == nullptr) return 0;   // neither gradient is wanted
    hipLaunchKernelGGL(aa_opacity_bwd_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n,
                       opacity_logits, compensation, v_opacities, v_opacity_logits, v_compensation);
    SGN_LAUNCH_CHECK();
    return 0;
}
