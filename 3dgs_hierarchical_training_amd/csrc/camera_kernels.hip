// camera_kernels.hip -- a frame's camera from its pose, and the virtual view between two poses, on the device.
//
// The reference builds a new `Camera` on the host for every iteration (/root/reference/scene/cameras.py:76-98, reached through
// `load_viewpoint_cam`, /root/reference/trainer/trainer.py:989-1142): a transpose, four small uploads, a `bmm` and `inverse()` of a 4x4 on
// the device, which waits for it.  The virtual views of the non-leaf phase add `get_virtual_view`
// (/root/reference/trainer/ht3dgs_trainer.py:462-479): a group logarithm, a scaled exponential and two products, ~50 tiny launches or
// host operations.  Both are a few hundred float64 operations on sixteen numbers; here each is ONE launch of one wave, fed by a pose that
// never leaves the device.  Semantics (operation order included) are pinned in include/gsr.h; tests/camera_device_common.py restates them in
// numpy float64.
//
//   gsr_camera_from_pose    lane b builds camera b of B <= 16: view = pose^T (a copy), full projection = view * P^T as four-term sums,
//                           camera centre = -(adj(A) t) / det(A).  float64 throughout, one rounding to float32 per output.
//   gsr_pose_virtual_view   lane 0: pose0 * Exp(alpha * Log(pose0^-1 * pose1)) and, with a base pose, that times base^-1.  float64.
//
// Nothing here may contract to an FMA: the float64 results are then the ones of the same statements evaluated on the host, and an entry that
// is exactly 0 or 1 there is exactly 0 or 1 here.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "../../include/gsr.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int kCamMaxBatch = 16;

struct CamProjection { double P[16]; };     // the projection matrix, row-major, as /root/reference/scene/cameras.py:87-90 writes it

// adjugate and determinant of the 3x3 block of a row-major 4x4: inverse(A) = adj / det
__device__ inline double adj3(const double* m, double* adj)
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    adj[0] = a11 * a22 - a12 * a21;  adj[1] = a02 * a21 - a01 * a22;  adj[2] = a01 * a12 - a02 * a11;
    adj[3] = a12 * a20 - a10 * a22;  adj[4] = a00 * a22 - a02 * a20;  adj[5] = a02 * a10 - a00 * a12;
    adj[6] = a10 * a21 - a11 * a20;  adj[7] = a01 * a20 - a00 * a21;  adj[8] = a00 * a11 - a01 * a10;
    return (a00 * adj[0] + a01 * adj[3]) + a02 * adj[6];
}

__global__ __launch_bounds__(64) void k_camera_from_pose(const float* __restrict__ pose, int B, CamProjection pr, float* __restrict__ viewmatrix,
                                                         float* __restrict__ projmatrix, float* __restrict__ campos)
{
    const int b = threadIdx.x;
    if (b >= B) return;
    double p[16];
    for (int k = 0; k < 16; ++k) p[k] = (double)pose[16 * b + k];
    // world_view_transform = pose^T (cameras.py:78-80)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) viewmatrix[16 * b + 4 * i + j] = pose[16 * b + 4 * j + i];
    // full_proj_transform = view bmm projection^T (cameras.py:97): entry (i,j) = sum_k pose[k][i] * P[j][k], k ascending
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double s = ((p[i] * pr.P[4 * j] + p[4 + i] * pr.P[4 * j + 1]) + p[8 + i] * pr.P[4 * j + 2]) + p[12 + i] * pr.P[4 * j + 3];
            projmatrix[16 * b + 4 * i + j] = (float)s;
        }
    // camera_center = world_view_transform.inverse()[3, :3] (cameras.py:98) = -A^-1 t; A is not assumed orthonormal
    double adj[9];
    const double det = adj3(p, adj);
    const double t0 = p[3], t1 = p[7], t2 = p[11];
    for (int i = 0; i < 3; ++i)
        campos[3 * b + i] = (float)(-(((adj[3 * i] * t0 + adj[3 * i + 1] * t1) + adj[3 * i + 2] * t2) / det));
}

// ---- rigid 3x4 algebra in float64 (row-major 4x4 storage, the last row taken as (0,0,0,1)) ---------------------------------------------
__device__ inline void affine_inverse(const double* m, double* out)
{
    double adj[9];
    const double det = adj3(m, adj);
    double inv[9];
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[4 * i + j] = inv[3 * i + j];
        out[4 * i + 3] = -((inv[3 * i] * m[3] + inv[3 * i + 1] * m[7]) + inv[3 * i + 2] * m[11]);
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
}

__device__ inline void affine_mul(const double* x, const double* y, double* out)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (x[4 * i] * y[j] + x[4 * i + 1] * y[4 + j]) + x[4 * i + 2] * y[8 + j];
        out[4 * i + 3] = ((x[4 * i] * y[3] + x[4 * i + 1] * y[7]) + x[4 * i + 2] * y[11]) + x[4 * i + 3];
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
}

// Rodrigues rotation R = exp(phi^) and the left Jacobian V (t = V tau), row-major 3x3; the series below theta^2 = 1e-8 (pose.so3_exp_and_v)
__device__ inline void so3_exp_and_v(const double* phi, double* R, double* V)
{
    const double th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
    double a, b, c;
    if (th2 < 1e-8) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
        c = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
        c = (th - sin(th)) / (th2 * th);
    }
    const double K[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
    double K2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
    for (int k = 0; k < 9; ++k) {
        const double eye = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        R[k] = (eye + a * K[k]) + b * K2[k];
        V[k] = (eye + b * K[k]) + c * K2[k];
    }
}

__global__ __launch_bounds__(64) void k_pose_virtual_view(const float* __restrict__ pose0, const float* __restrict__ pose1, double alpha,
                                                          const float* __restrict__ base, float* __restrict__ out, float* __restrict__ out_rel)
{
    if (threadIdx.x != 0) return;
    double p0[16], p1[16], inv0[16], rel[16];
    for (int k = 0; k < 16; ++k) { p0[k] = (double)pose0[k]; p1[k] = (double)pose1[k]; }
    affine_inverse(p0, inv0);
    affine_mul(inv0, p1, rel);
    // Log: the rotation vector (pose.so3_log, series below theta = 1e-4), then tau = V^-1 t by the adjugate
    double cosv = (((rel[0] + rel[5]) + rel[10]) - 1.0) * 0.5;
    cosv = cosv < -1.0 ? -1.0 : (cosv > 1.0 ? 1.0 : cosv);
    const double th = acos(cosv);
    const double k = th < 1e-4 ? 1.0 + th * th / 6.0 : th / sin(th);
    double xi[6];
    xi[3] = k * ((rel[9] - rel[6]) * 0.5);
    xi[4] = k * ((rel[2] - rel[8]) * 0.5);
    xi[5] = k * ((rel[4] - rel[1]) * 0.5);
    double R[9], V[9], V4[16], adj[9];
    so3_exp_and_v(xi + 3, R, V);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V4[4 * i + j] = V[3 * i + j];
    const double det = adj3(V4, adj);
    for (int i = 0; i < 3; ++i) xi[i] = ((adj[3 * i] * rel[3] + adj[3 * i + 1] * rel[7]) + adj[3 * i + 2] * rel[11]) / det;
    // Exp(alpha * xi)
    for (int i = 0; i < 6; ++i) xi[i] = alpha * xi[i];
    so3_exp_and_v(xi + 3, R, V);
    double E[16], o[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) E[4 * i + j] = R[3 * i + j];
        E[4 * i + 3] = (V[3 * i] * xi[0] + V[3 * i + 1] * xi[1]) + V[3 * i + 2] * xi[2];
    }
    E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
    affine_mul(p0, E, o);
    for (int i = 0; i < 16; ++i) out[i] = (float)o[i];
    if (base) {
        double bs[16], binv[16], r[16];
        for (int i = 0; i < 16; ++i) bs[i] = (double)base[i];
        affine_inverse(bs, binv);
        affine_mul(o, binv, r);
        for (int i = 0; i < 16; ++i) out_rel[i] = (float)r[i];
    }
}

}  // namespace gsr

extern "C" {

int gsr_camera_from_pose(const float* pose, int32_t B, double fx, double fy, double cx, double cy, int32_t W, int32_t H, double znear,
                         double zfar, float* viewmatrix, float* projmatrix, float* campos, void* stream)
{
    if (!pose || !viewmatrix || !projmatrix || !campos) return GSR_ERR_ARG;
    if (B < 1 || B > gsr::kCamMaxBatch || W <= 0 || H <= 0) return GSR_ERR_ARG;
    if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return GSR_ERR_ARG;
    if (!std::isfinite(znear) || !std::isfinite(zfar) || zfar == znear) return GSR_ERR_ARG;
    gsr::CamProjection pr;
    for (int k = 0; k < 16; ++k) pr.P[k] = 0.0;
    const double w = (double)W, h = (double)H;
    pr.P[0] = 2.0 * fx / w;
    pr.P[2] = -(w - 2.0 * cx) / w;
    pr.P[5] = 2.0 * fy / h;
    pr.P[6] = -(h - 2.0 * cy) / h;
    pr.P[10] = zfar / (zfar - znear);
    pr.P[11] = -(zfar * znear) / (zfar - znear);
    pr.P[14] = 1.0;
    hipLaunchKernelGGL(gsr::k_camera_from_pose, dim3(1), dim3(64), 0, (hipStream_t)stream, pose, (int)B, pr, viewmatrix, projmatrix, campos);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_pose_virtual_view(const float* pose0, const float* pose1, double alpha, const float* base, float* out, float* out_rel, void* stream)
{
    if (!pose0 || !pose1 || !out) return GSR_ERR_ARG;
    if ((base != nullptr) != (out_rel != nullptr)) return GSR_ERR_ARG;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return GSR_ERR_ARG;
    hipLaunchKernelGGL(gsr::k_pose_virtual_view, dim3(1), dim3(64), 0, (hipStream_t)stream, pose0, pose1, alpha, base, out, out_rel);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
