// rolling_shutter.hip — rolling-shutter compensation of the projection's outputs, gfx950.
//
// A street camera reads its sensor row by row (or column by column) over tens of milliseconds while the vehicle and the
// tracked objects move.  To first order a Gaussian's centre crosses the image at a constant velocity `a` during the
// readout, and what the rolling sensor records of it is again an exact Gaussian: the centre shifted to where the
// shutter meets it, the conic sheared by a 2x2 matrix.  This pair applies that to (xys, depths, radii, conics,
// num_tiles_hit) directly behind the projection; binning, the rasterizers and every later pass run on what comes out.
// Pure streaming: one row per lane, 4-byte coalesced accesses (n is arbitrary and the tensors may be 4-byte-aligned
// slices of an arena), no LDS, no atomics; 60 bytes per row forward (64 with object ids; the velocity table is a few
// cache lines), at most 56 in and 24 out backward.
// The arithmetic is a contract (include/sgn_rast.h "ROLLING SHUTTER"): fp32, no contraction, the expressions in the
// order written there — with no motion every product below is with an exact 0 or 1 and every output equals its input
// bit for bit.
#include "sgn_common.h"

namespace {

struct Row {                 // what forward and backward both derive from one input row
    float ux, uy, z;         // centre on the real pixel grid (margin taken off), depth
    float x, y;              // camera-space mean
    float pdx, pdy, pdz;     // point velocity in the camera frame
    float ax, ay;            // screen velocity, px / s
    float go, gs;            // g = a T / E: its other-axis and shutter-axis entries
    float b, k;              // A's two non-trivial entries: -g_other and 1 - g_shutter
    float us1, tau1;         // sheared shutter-axis coordinate, its time
};

__device__ __forceinline__ void rs_velocity(const sgn_shutter &rs, const int32_t *object_ids, const float *lin_table,
                                            int n_objects, int i, float (&l)[3]) {
    l[0] = rs.lin[0]; l[1] = rs.lin[1]; l[2] = rs.lin[2];
    if (object_ids != nullptr) {
        const int id = min(max(object_ids[i], 0), n_objects - 1);      // an id outside the table reads its nearest row
        l[0] = lin_table[3 * id]; l[1] = lin_table[3 * id + 1]; l[2] = lin_table[3 * id + 2];
    }
}

__device__ __forceinline__ Row rs_row(const sgn_shutter &rs, const float (&l)[3], float u0, float u1, float z) {
    Row r;
    r.ux = u0 - rs.margin; r.uy = u1 - rs.margin; r.z = z;
    const float zz = z + 1e-6f;
    r.x = (r.ux - rs.cx) * zz / rs.fx;
    r.y = (r.uy - rs.cy) * zz / rs.fy;
    const float wx = rs.ang[0], wy = rs.ang[1], wz = rs.ang[2];
    r.pdx = -l[0] - (wy * z - wz * r.y);
    r.pdy = -l[1] - (wz * r.x - wx * z);
    r.pdz = -l[2] - (wx * r.y - wy * r.x);
    r.ax = rs.fx * (r.pdx - (r.x / z) * r.pdz) / z;
    r.ay = rs.fy * (r.pdy - (r.y / z) * r.pdz) / z;
    const float extent = (float)(rs.axis == SGN_SHUTTER_ROWS ? rs.img_h : rs.img_w);
    const float gx = r.ax * rs.duration / extent, gy = r.ay * rs.duration / extent;
    const float gs = rs.axis == SGN_SHUTTER_ROWS ? gy : gx, go = rs.axis == SGN_SHUTTER_ROWS ? gx : gy;
    const float as = rs.axis == SGN_SHUTTER_ROWS ? r.ay : r.ax, us = rs.axis == SGN_SHUTTER_ROWS ? r.uy : r.ux;
    r.go = go; r.gs = gs;
    r.k = 1.f - gs;
    r.b = -go;
    r.us1 = (us - 0.5f * rs.duration * as) / r.k;
    r.tau1 = rs.duration * (r.us1 / extent - 0.5f);
    return r;
}

__global__ __launch_bounds__(256) void rolling_shutter_fwd_kernel(
    int n, const float *__restrict__ xys, const float *__restrict__ depths, const int32_t *__restrict__ radii,
    const float *__restrict__ conics, const int32_t *__restrict__ object_ids, const float *__restrict__ lin_table,
    int n_objects, const sgn_shutter rs, int tiles_x, int tiles_y, float *__restrict__ xys_out,
    float *__restrict__ depths_out, int32_t *__restrict__ radii_out, float *__restrict__ conics_out,
    int32_t *__restrict__ num_tiles_hit_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int rad = radii[i];
    const float q0 = conics[3 * i], q1 = conics[3 * i + 1], q2 = conics[3 * i + 2];
    float o_x = 0.f, o_y = 0.f, o_d = 0.f, o_q0 = q0, o_q1 = q1, o_q2 = q2;      // a row the projection culled keeps its conic
    int o_r = 0, o_n = 0;
    if (rad > 0) {
        float l[3];
        rs_velocity(rs, object_ids, lin_table, n_objects, i, l);
        const Row r = rs_row(rs, l, xys[2 * i], xys[2 * i + 1], depths[i]);
        const bool rows = rs.axis == SGN_SHUTTER_ROWS;
        const float uo = rows ? r.ux : r.uy, ao = rows ? r.ax : r.ay;
        const float uo1 = uo + ao * r.tau1;
        const float d1 = r.z + r.pdz * r.tau1;
        // Q' = A^T Q A with A e_other = e_other, A e_shutter = b e_other + k e_shutter
        const float qoo = rows ? q0 : q2, qss = rows ? q2 : q0;
        const float qos1 = qoo * r.b + q1 * r.k;
        const float qss1 = r.b * qos1 + r.k * (q1 * r.b + qss * r.k);
        o_q0 = rows ? qoo : qss1; o_q1 = qos1; o_q2 = rows ? qss1 : qoo;
        // sigma: the largest singular value of A^-1 = [[1, c], [0, d]] (up to the axes' order), c = g_other / k
        const float c = r.go / r.k, d = 1.f + r.gs / r.k;
        const float t = 1.f + c * c + d * d;
        const float sigma = sqrtf(0.5f * (t + sqrtf(fmaxf(0.f, t * t - 4.f * (d * d)))));
        const float radius = ceilf((float)rad * sigma);
        const float x1 = rows ? uo1 : r.us1, y1 = rows ? r.us1 : uo1;
        int mnx, mny, mxx, mxy;
        sgn_tile_bbox(x1, y1, radius, tiles_x, tiles_y, rs.block_width, mnx, mny, mxx, mxy, rs.semantics);
        const int area = (mxx - mnx) * (mxy - mny);
        if (!(r.k < 0.5f) && d1 > rs.clip_thresh && area > 0) {
            o_x = x1; o_y = y1; o_d = d1; o_r = sgn_f2i(radius); o_n = area;
        }
    }
    xys_out[2 * i] = o_x; xys_out[2 * i + 1] = o_y;
    depths_out[i] = o_d;
    radii_out[i] = o_r;
    conics_out[3 * i] = o_q0; conics_out[3 * i + 1] = o_q1; conics_out[3 * i + 2] = o_q2;
    num_tiles_hit_out[i] = o_n;
}

// v_depths_out may be NULL.  A row whose forward output was culled (radii_out <= 0) gets zero gradients.
__global__ __launch_bounds__(256) void rolling_shutter_bwd_kernel(
    int n, const float *__restrict__ xys, const float *__restrict__ depths, const float *__restrict__ conics,
    const int32_t *__restrict__ radii_out, const int32_t *__restrict__ object_ids, const float *__restrict__ lin_table,
    int n_objects, const sgn_shutter rs, const float *__restrict__ v_xys_out, const float *__restrict__ v_depths_out,
    const float *__restrict__ v_conics_out, float *__restrict__ v_xys, float *__restrict__ v_depths,
    float *__restrict__ v_conics) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float g_ux = 0.f, g_uy = 0.f, g_z = 0.f, g_q0 = 0.f, g_q1 = 0.f, g_q2 = 0.f;
    if (radii_out[i] > 0) {
        float l[3];
        rs_velocity(rs, object_ids, lin_table, n_objects, i, l);
        const Row r = rs_row(rs, l, xys[2 * i], xys[2 * i + 1], depths[i]);
        const bool rows = rs.axis == SGN_SHUTTER_ROWS;
        const float extent = (float)(rows ? rs.img_h : rs.img_w);
        const float T = rs.duration, te = T / extent, z = r.z;
        const float q0 = conics[3 * i], q1 = conics[3 * i + 1], q2 = conics[3 * i + 2];
        const float qoo = rows ? q0 : q2, qss = rows ? q2 : q0;
        const float vx1 = v_xys_out[2 * i], vy1 = v_xys_out[2 * i + 1];
        const float vd1 = v_depths_out != nullptr ? v_depths_out[i] : 0.f;
        const float vq0 = v_conics_out[3 * i], vq1 = v_conics_out[3 * i + 1], vq2 = v_conics_out[3 * i + 2];
        const float vo1 = rows ? vx1 : vy1, vs1 = rows ? vy1 : vx1;
        const float voo1 = rows ? vq0 : vq2, vss1 = rows ? vq2 : vq0, vos1 = vq1;
        const float ao = rows ? r.ax : r.ay;
        // u'_other = u_other + a_other tau', depth' = z + pd_z tau'
        const float v_tau = vo1 * ao + vd1 * r.pdz;
        float v_ao = vo1 * r.tau1;
        float v_pdz = vd1 * r.tau1;
        float v_z = vd1;
        const float v_uo = vo1;
        // tau' = T (u'_s / E - 0.5), u'_s = (u_s - 0.5 T a_s) / k
        const float v_us1 = vs1 + v_tau * te;
        const float v_us = v_us1 / r.k;
        float v_as = v_us1 * (-0.5f * T) / r.k;
        float v_k = -v_us1 * r.us1 / r.k;
        // Q'_oo = Q_oo, Q'_os = b Q_oo + k Q_os, Q'_ss = b^2 Q_oo + 2 b k Q_os + k^2 Q_ss
        const float b = r.b, k = r.k;
        const float g_oo = voo1 + b * vos1 + b * b * vss1;
        const float g_os = k * vos1 + 2.f * b * k * vss1;
        const float g_ss = k * k * vss1;
        const float v_b = qoo * vos1 + 2.f * (b * qoo + k * q1) * vss1;
        v_k += q1 * vos1 + 2.f * (b * q1 + k * qss) * vss1;
        g_q0 = rows ? g_oo : g_ss; g_q1 = g_os; g_q2 = rows ? g_ss : g_oo;
        // b = -a_other T / E, k = 1 - a_s T / E
        v_ao -= v_b * te;
        v_as -= v_k * te;
        const float v_ax = rows ? v_ao : v_as, v_ay = rows ? v_as : v_ao;
        // a_x = fx (pd_x - (x / z) pd_z) / z, a_y alike
        const float rz = 1.f / z, rz2 = rz * rz;
        const float fxz = v_ax * rs.fx * rz, fyz = v_ay * rs.fy * rz;
        float v_pdx = fxz, v_pdy = fyz;
        v_pdz -= fxz * r.x * rz + fyz * r.y * rz;
        float v_x = -fxz * r.pdz * rz, v_y = -fyz * r.pdz * rz;
        v_z += -v_ax * r.ax * rz + fxz * r.x * r.pdz * rz2 - v_ay * r.ay * rz + fyz * r.y * r.pdz * rz2;
        // pd = -l - w x p
        const float wx = rs.ang[0], wy = rs.ang[1], wz = rs.ang[2];
        v_z += -wy * v_pdx + wx * v_pdy;
        v_y += wz * v_pdx - wx * v_pdz;
        v_x += -wz * v_pdy + wy * v_pdz;
        // x = (u_x - cx) (z + 1e-6) / fx, y alike
        const float zz = z + 1e-6f;
        const float v_ux_p = v_x * zz / rs.fx, v_uy_p = v_y * zz / rs.fy;
        v_z += v_x * (r.ux - rs.cx) / rs.fx + v_y * (r.uy - rs.cy) / rs.fy;
        g_ux = v_ux_p + (rows ? v_uo : v_us);
        g_uy = v_uy_p + (rows ? v_us : v_uo);
        g_z = v_z;
    }
    v_xys[2 * i] = g_ux; v_xys[2 * i + 1] = g_uy;
    v_depths[i] = g_z;
    v_conics[3 * i] = g_q0; v_conics[3 * i + 1] = g_q1; v_conics[3 * i + 2] = g_q2;
}

// the checks both entries share; `fn` is the public entry's name
int rs_check(const char *fn, int n, const int32_t *object_ids, const float *lin_table, int n_objects,
             const sgn_shutter *rs) {
    SGN_ARG_CHECK_FN(fn, n >= 0, -1);
    SGN_ARG_CHECK_FN(fn, rs != nullptr, -2);
    SGN_ARG_CHECK_FN(fn, rs->axis == SGN_SHUTTER_ROWS || rs->axis == SGN_SHUTTER_COLS, -3);
    SGN_ARG_CHECK_FN(fn, rs->img_h >= 1 && rs->img_w >= 1 && rs->block_width > 1 && rs->block_width <= 16, -4);
    SGN_ARG_CHECK_FN(fn, rs->fx > 0.f && rs->fy > 0.f && rs->margin >= 0.f, -5);
    SGN_ARG_CHECK_FN(fn, (object_ids == nullptr) == (lin_table == nullptr), -6);
    SGN_ARG_CHECK_FN(fn, object_ids == nullptr || n_objects >= 1, -6);
    return 0;
}

}  // namespace

SGN_EXPORT int sgn_rolling_shutter_fwd(int n, const float *xys, const float *depths, const int32_t *radii,
                                       const float *conics, const int32_t *object_ids, const float *lin_table,
                                       int n_objects, const sgn_shutter *rs, float *xys_out, float *depths_out,
                                       int32_t *radii_out, float *conics_out, int32_t *num_tiles_hit_out,
                                       sgn_stream_t stream) {
    const int rc = rs_check(__func__, n, object_ids, lin_table, n_objects, rs);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    SGN_ARG_CHECK(xys && depths && radii && conics && xys_out && depths_out && radii_out && conics_out &&
                      num_tiles_hit_out, -2);
    const int tiles_x = (rs->img_w + rs->block_width - 1) / rs->block_width;
    const int tiles_y = (rs->img_h + rs->block_width - 1) / rs->block_width;
    hipLaunchKernelGGL(rolling_shutter_fwd_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, xys,
                       depths, radii, conics, object_ids, lin_table, n_objects, *rs, tiles_x, tiles_y, xys_out,
                       depths_out, radii_out, conics_out, num_tiles_hit_out);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_rolling_shutter_bwd(int n, const float *xys, const float *depths, const float *conics,
                                       const int32_t *radii_out, const int32_t *object_ids, const float *lin_table,
                                       int n_objects, const sgn_shutter *rs, const float *v_xys_out,
                                       const float *v_depths_out, const float *v_conics_out, float *v_xys,
                                       float *v_depths, float *v_conics, sgn_stream_t stream) {
    const int rc = rs_check(__func__, n, object_ids, lin_table, n_objects, rs);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    SGN_ARG_CHECK(xys && depths && conics && radii_out && v_xys_out && v_conics_out && v_xys && v_depths && v_conics,
                  -2);
    hipLaunchKernelGGL(rolling_shutter_bwd_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, xys,
                       depths, conics, radii_out, object_ids, lin_table, n_objects, *rs, v_xys_out, v_depths_out,
                       v_conics_out, v_xys, v_depths, v_conics);
    SGN_LAUNCH_CHECK();
    return 0;
}
