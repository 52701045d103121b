// optim_kernels.hip -- multi-tensor Adam step in ONE launch ("next" row f-2 of SURVEY.md section 8).
//
// The reference updates its six parameter groups with torch.optim.Adam(l, lr=0.0, eps=1e-15)
// (/root/reference/scene/gaussian_model_ht.py:275-289; per-group learning rates
// /root/reference/arguments/__init__.py:116-131).  That is 59 floats per Gaussian; the update is a pure HBM
// stream: read p, g, m, v and write p, m, v = 28 B per float = 1652 B per Gaussian.  This kernel walks all groups
// in a single grid with 16-byte accesses.  Update rule = torch's (non-amsgrad, no weight decay):
//   m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/gsr.h"
#include "adam_math.h"

namespace gsr {

constexpr int kAdamThreads = 256;
constexpr int kAdamVec = 4;                 // floats per thread per step (16-byte accesses)
constexpr int kAdamChunk = kAdamThreads * kAdamVec * 4;   // floats per block

struct AdamBatch {
    GsrAdamTensor t[GSR_ADAM_MAX_TENSORS];
    uint32_t block_start[GSR_ADAM_MAX_TENSORS + 1];
    int count;
    float beta1, beta2, eps, bc1, bc2_sqrt;
};

__global__ __launch_bounds__(kAdamThreads) void k_adam(AdamBatch B)
{
    int ti = 0;
#pragma unroll
    for (int k = 1; k < GSR_ADAM_MAX_TENSORS; k++)
        if (k < B.count && blockIdx.x >= B.block_start[k]) ti = k;
    const GsrAdamTensor t = B.t[ti];
    const uint64_t base = (uint64_t)(blockIdx.x - B.block_start[ti]) * kAdamChunk;
    const float step_size = t.lr / B.bc1, inv_bc2s = 1.f / B.bc2_sqrt;
    const bool aligned = ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15) == 0);
    // whole, aligned chunks: the four turns' sixteen loads are requested before the first turn is computed (the update is in place, so
    // the compiler must take a later turn's loads for may-aliases of an earlier turn's stores and, left to itself, runs the turns one
    // memory round trip after the other -- vmcnt counts loads and stores alike on gfx9)
    if (aligned && base + kAdamChunk <= t.n) {
        float4 p[4], g[4], m[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint64_t i = base + (uint64_t)(r * kAdamThreads + threadIdx.x) * kAdamVec;
            p[r] = nt_load4(reinterpret_cast<const float4*>(t.param + i));
            g[r] = nt_load4(reinterpret_cast<const float4*>(t.grad + i));
            m[r] = nt_load4(reinterpret_cast<const float4*>(t.exp_avg + i));
            v[r] = nt_load4(reinterpret_cast<const float4*>(t.exp_avg_sq + i));
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint64_t i = base + (uint64_t)(r * kAdamThreads + threadIdx.x) * kAdamVec;
            const float4 p0 = p[r], m0 = m[r], v0 = v[r];
            adam_one(p[r].x, g[r].x, m[r].x, v[r].x, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p[r].y, g[r].y, m[r].y, v[r].y, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p[r].z, g[r].z, m[r].z, v[r].z, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p[r].w, g[r].w, m[r].w, v[r].w, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            // the update is in place: a 128-byte line (eight lanes' elements) it left bit for bit as loaded is already in memory
            // (adam_unchanged4 / adam_line_changed, adam_math.h)
            if (!adam_line_changed<8>(!adam_unchanged4(p0, m0, v0, p[r], m[r], v[r]), (int)(threadIdx.x & 63))) continue;
            nt_store4(reinterpret_cast<float4*>(t.param + i), p[r]);
            nt_store4(reinterpret_cast<float4*>(t.exp_avg + i), m[r]);
            nt_store4(reinterpret_cast<float4*>(t.exp_avg_sq + i), v[r]);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint64_t i = base + (uint64_t)(r * kAdamThreads + threadIdx.x) * kAdamVec;
        if (i >= t.n) break;
        if (aligned && i + kAdamVec <= t.n) {
            float4 p = nt_load4(reinterpret_cast<const float4*>(t.param + i));
            const float4 g = nt_load4(reinterpret_cast<const float4*>(t.grad + i));
            float4 m = nt_load4(reinterpret_cast<const float4*>(t.exp_avg + i));
            float4 v = nt_load4(reinterpret_cast<const float4*>(t.exp_avg_sq + i));
            const float4 p0 = p, m0 = m, v0 = v;
            adam_one(p.x, g.x, m.x, v.x, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p.y, g.y, m.y, v.y, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p.z, g.z, m.z, v.z, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            adam_one(p.w, g.w, m.w, v.w, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
            if (!adam_line_changed<8>(!adam_unchanged4(p0, m0, v0, p, m, v), (int)(threadIdx.x & 63))) continue;
            nt_store4(reinterpret_cast<float4*>(t.param + i), p);
            nt_store4(reinterpret_cast<float4*>(t.exp_avg + i), m);
            nt_store4(reinterpret_cast<float4*>(t.exp_avg_sq + i), v);
        } else {
            for (uint64_t k = i; k < t.n && k < i + kAdamVec; k++) {
                float p = t.param[k], m = t.exp_avg[k], v = t.exp_avg_sq[k];
                const float p0 = p, m0 = m, v0 = v;
                adam_one(p, t.grad[k], m, v, B.beta1, B.beta2, B.eps, step_size, inv_bc2s);
                if (adam_unchanged(p0, m0, v0, p, m, v)) continue;
                t.param[k] = p; t.exp_avg[k] = m; t.exp_avg_sq[k] = v;
            }
        }
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_adam_step(const GsrAdamTensor* tensors, int32_t count, float beta1, float beta2, float eps, int64_t step,
                             void* stream)
{
    if (!tensors || count <= 0 || count > GSR_ADAM_MAX_TENSORS || step <= 0) return GSR_ERR_ARG;
    AdamBatch B;
    uint32_t blocks = 0;
    for (int k = 0; k < count; k++) {
        B.t[k] = tensors[k];
        if (tensors[k].n && (!tensors[k].param || !tensors[k].grad || !tensors[k].exp_avg || !tensors[k].exp_avg_sq)) return GSR_ERR_ARG;
        B.block_start[k] = blocks;
        blocks += (uint32_t)((tensors[k].n + kAdamChunk - 1) / kAdamChunk);
    }
    for (int k = count; k <= GSR_ADAM_MAX_TENSORS; k++) B.block_start[k] = blocks;
    B.count = count; B.beta1 = beta1; B.beta2 = beta2; B.eps = eps;
    B.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    B.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    if (blocks == 0) return GSR_OK;
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(kAdamThreads), 0, (hipStream_t)stream, B);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

// ------------------------------------------------------------------------------------------------
// Pose step of stage A (compute_relative_pose, /root/reference/trainer/ht3dgs_trainer.py:308-333, :367-378): the camera
// pose is the group element Exp(delta) * B with six tangent numbers delta = (tau, phi) under Adam
// (`LieGroupParameter.retr()` + torch.optim.Adam in the reference).  One iteration of that loop in torch is ~50 tiny
// kernels (exponential map, its autograd, the optimizer) -- 1.9 ms of launch latency around a 0.35 ms render at 130 k
// Gaussians.  Here it is ONE one-thread kernel between two renders: it takes dL/dM (12 floats, from gsr_backward's
// d_points_transform), chains it to dL/d(delta), applies torch's Adam update to delta and writes the next M = Exp(delta) B
// where the next render reads its points_transform.  Same statement of the exponential map as pose.py (Rodrigues + left
// Jacobian, series near 0), evaluated in float64; its Jacobian by central differences in float64 (h = 1e-6: error ~1e-10,
// far below the float32 gradient it multiplies).  Adam arithmetic in float32, as torch does it for a float32 parameter.
// ------------------------------------------------------------------------------------------------
namespace gsr {

__device__ inline void se3_exp_times(const double* d /*6*/, const double* B /*12, row-major 3x4, or nullptr = identity*/, double* M /*12*/)
{
    const double tx = d[0], ty = d[1], tz = d[2], px = d[3], py = d[4], pz = d[5];
    const double th2 = px * px + py * py + pz * pz;
    double a, b, c;
    if (th2 < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; c = 1.0 / 6.0 - th2 / 120.0; }
    else { const double th = sqrt(th2); a = sin(th) / th; b = (1.0 - cos(th)) / th2; c = (th - sin(th)) / (th2 * th); }
    const double K[9] = {0, -pz, py, pz, 0, -px, -py, px, 0};
    double K2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    double R[9], V[9];
    for (int q = 0; q < 9; q++) { const double e = (q % 4 == 0) ? 1.0 : 0.0; R[q] = e + a * K[q] + b * K2[q]; V[q] = e + b * K[q] + c * K2[q]; }
    const double t[3] = {V[0] * tx + V[1] * ty + V[2] * tz, V[3] * tx + V[4] * ty + V[5] * tz, V[6] * tx + V[7] * ty + V[8] * tz};
    for (int i = 0; i < 3; i++) {
        if (B) {
            for (int j = 0; j < 4; j++)
                M[4 * i + j] = R[3 * i] * B[j] + R[3 * i + 1] * B[4 + j] + R[3 * i + 2] * B[8 + j] + (j == 3 ? t[i] : 0.0);
        } else {
            M[4 * i] = R[3 * i]; M[4 * i + 1] = R[3 * i + 1]; M[4 * i + 2] = R[3 * i + 2]; M[4 * i + 3] = t[i];
        }
    }
}

// One 64-lane wave; lanes 0..11 evaluate the twelve perturbed exponential maps of the central differences side by side (a
// float64 sin / cos pair is a few hundred instructions: 13 maps in ONE lane took 33 us, the dependent chain of every step)
__device__ inline void pose_grad_and_adam(double* d /*6, lane-uniform copy*/, const double* Bp, const double* G /*12*/, float* __restrict__ delta,
                                          float* __restrict__ m, float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1,
                                          float bc2_sqrt, double (*s_M)[12], float* s_g)
{
    const int lane = threadIdx.x;
    const double h = 1e-6;
    if (lane < 12) {
        double dd[6];
        for (int k = 0; k < 6; k++) dd[k] = d[k];
        dd[lane >> 1] += (lane & 1) ? -h : h;
        se3_exp_times(dd, Bp, s_M[lane]);
    }
    __syncthreads();
    if (lane < 6) {
        double acc = 0.0;
        for (int q = 0; q < 12; q++) acc += G[q] * (s_M[2 * lane][q] - s_M[2 * lane + 1][q]) / (2.0 * h);
        const float g = (float)acc;
        const float mk = b1 * m[lane] + (1.f - b1) * g;          // torch.optim.Adam, single tensor, float32
        const float vk = b2 * v[lane] + (1.f - b2) * g * g;
        m[lane] = mk; v[lane] = vk;
        const float denom = sqrtf(vk) / bc2_sqrt + eps;
        const float p = delta[lane] - (lr / bc1) * (mk / denom);
        delta[lane] = p;
        s_g[lane] = p;
    }
    __syncthreads();
    for (int k = 0; k < 6; k++) d[k] = (double)s_g[k];
}

// MANY (gsr_pose_step_many): P poses, one workgroup each -- pose p at p * 6 / p * 12 floats; the poses share nothing but the hyper-parameters.
// One statement of the step for both, so that a pose gets the same bits from either; MANY = false is the kernel as it was.
template <bool MANY = false>
__global__ __launch_bounds__(64) void k_pose_adam(float* __restrict__ delta, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ d_xf, const float* __restrict__ base, float* __restrict__ xf_out,
                                                   float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt, int do_step)
{
    if constexpr (MANY) {
        const size_t p = blockIdx.x;
        delta += 6 * p; xf_out += 12 * p;
        if (m) m += 6 * p;
        if (v) v += 6 * p;
        if (d_xf) d_xf += 12 * p;
        if (base) base += 12 * p;
    }
    __shared__ double s_M[12][12];
    __shared__ float s_g[6];
    double d[6], B[12], G[12];
    for (int k = 0; k < 6; k++) d[k] = (double)delta[k];
    if (base) for (int q = 0; q < 12; q++) B[q] = (double)base[q];
    const double* Bp = base ? B : nullptr;
    __syncthreads();      // every lane has read delta before lanes 0..5 overwrite it
    if (do_step) {
        for (int q = 0; q < 12; q++) G[q] = (double)d_xf[q];
        pose_grad_and_adam(d, Bp, G, delta, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, s_M, s_g);
    }
    if (threadIdx.x == 0) {
        double M[12];
        se3_exp_times(d, Bp, M);
        for (int q = 0; q < 12; q++) xf_out[q] = (float)M[q];
    }
}

}  // namespace gsr

extern "C" int gsr_pose_step_many(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_points_transform12, const float* base12,
                                  float* points_transform_out12, int32_t P, float lr, float beta1, float beta2, float eps, int64_t step,
                                  void* stream)
{
    if (!delta6 || !points_transform_out12 || step < 0 || P < 1 || P > 65535) return GSR_ERR_ARG;
    if (step > 0 && (!exp_avg6 || !exp_avg_sq6 || !d_points_transform12)) return GSR_ERR_ARG;
    const float bc1 = step > 0 ? (float)(1.0 - pow((double)beta1, (double)step)) : 1.f;
    const float bc2s = step > 0 ? (float)sqrt(1.0 - pow((double)beta2, (double)step)) : 1.f;
    hipLaunchKernelGGL(gsr::k_pose_adam<true>, dim3(P), dim3(64), 0, (hipStream_t)stream, delta6, exp_avg6, exp_avg_sq6, d_points_transform12,
                       base12, points_transform_out12, lr, beta1, beta2, eps, bc1, bc2s, step > 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

extern "C" int gsr_pose_step(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_points_transform12, const float* base12,
                             float* points_transform_out12, float lr, float beta1, float beta2, float eps, int64_t step, void* stream)
{
    if (!delta6 || !points_transform_out12 || step < 0) return GSR_ERR_ARG;
    if (step > 0 && (!exp_avg6 || !exp_avg_sq6 || !d_points_transform12)) return GSR_ERR_ARG;
    const float bc1 = step > 0 ? (float)(1.0 - pow((double)beta1, (double)step)) : 1.f;
    const float bc2s = step > 0 ? (float)sqrt(1.0 - pow((double)beta2, (double)step)) : 1.f;
    hipLaunchKernelGGL(gsr::k_pose_adam<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, delta6, exp_avg6, exp_avg_sq6, d_points_transform12, base12,
                       points_transform_out12, lr, beta1, beta2, eps, bc1, bc2s, step > 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

// The chain alone: dL/d(delta) of M = Exp(delta) * base from dL/dM, written to d_delta6_out -- the backward of the autograd node
// gsr_autopatch puts where the unmodified trainer's `P[k].retr()` stands (torch_ext.cpp PoseMatrixFn): the trainer's own
// optimizer object (its Adam over the frame's six numbers) then finds `.grad` where autograd always leaves it.  The same central
// differences in float64 as pose_grad_and_adam above.
namespace gsr {

__global__ __launch_bounds__(64) void k_pose_grad(const float* __restrict__ delta, const float* __restrict__ d_xf, const float* __restrict__ base,
                                                   float* __restrict__ d_delta)
{
    __shared__ double s_M[12][12];
    const int lane = threadIdx.x;
    double d[6], B[12];
    for (int k = 0; k < 6; k++) d[k] = (double)delta[k];
    if (base) for (int q = 0; q < 12; q++) B[q] = (double)base[q];
    const double h = 1e-6;
    if (lane < 12) {
        d[lane >> 1] += (lane & 1) ? -h : h;
        se3_exp_times(d, base ? B : nullptr, s_M[lane]);
    }
    __syncthreads();
    if (lane < 6) {
        double acc = 0.0;
        for (int q = 0; q < 12; q++) acc += (double)d_xf[q] * (s_M[2 * lane][q] - s_M[2 * lane + 1][q]) / (2.0 * h);
        d_delta[lane] = (float)acc;
    }
}

}  // namespace gsr

extern "C" int gsr_pose_grad(const float* delta6, const float* d_points_transform12, const float* base12, float* d_delta6_out, void* stream)
{
    if (!delta6 || !d_points_transform12 || !d_delta6_out) return GSR_ERR_ARG;
    hipLaunchKernelGGL(gsr::k_pose_grad, dim3(1), dim3(64), 0, (hipStream_t)stream, delta6, d_points_transform12, base12, d_delta6_out);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

// ------------------------------------------------------------------------------------------------
// The same pose step when the pose lives in the CAMERA of the render instead of a transform of the means: the render's
// three camera tensors are functions of the world-to-camera matrix M = Exp(delta) * base,
//   viewmatrix V = M^T,  projmatrix F = V * Pt (Pt = transposed projection, fixed intrinsics),  campos c = -R^T t,
// and gsr_backward returns dL/dV, dL/dF, dL/dc (d_viewmatrix / d_projmatrix / d_campos).  This kernel folds the three into
// dL/dM (rows 0..2), chains to dL/d(delta), applies Adam and rewrites V, F and c IN PLACE for the next render of the frame.
// View-dependent colour keeps its world-frame directions this way (with a transform of the means they would be taken in
// each camera's own frame).
// ------------------------------------------------------------------------------------------------
namespace gsr {

__global__ __launch_bounds__(64) void k_pose_adam_camera(float* __restrict__ delta, float* __restrict__ m, float* __restrict__ v,
                                                          const float* __restrict__ d_vm, const float* __restrict__ d_pm,
                                                          const float* __restrict__ d_cp, const float* __restrict__ projT,
                                                          const float* __restrict__ base, float* __restrict__ vm, float* __restrict__ pm,
                                                          float* __restrict__ cp, float lr, float b1, float b2, float eps, float bc1,
                                                          float bc2_sqrt, int do_step)
{
    __shared__ double s_M[12][12];
    __shared__ float s_g[6];
    double d[6], B[12], M[12], Pt[16];
    for (int k = 0; k < 6; k++) d[k] = (double)delta[k];
    if (base) for (int q = 0; q < 12; q++) B[q] = (double)base[q];
    for (int q = 0; q < 16; q++) Pt[q] = (double)projT[q];
    const double* Bp = base ? B : nullptr;
    __syncthreads();
    if (do_step) {
        se3_exp_times(d, Bp, M);
        // dL/dV_total = dV + dF Pt^T ;  dL/dM[i][j] = dL/dV_total[j][i]  (V = M^T)
        double G[12];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) {
                double a = d_vm ? (double)d_vm[4 * j + i] : 0.0;
                if (d_pm) for (int k = 0; k < 4; k++) a += (double)d_pm[4 * j + k] * Pt[4 * i + k];
                G[4 * i + j] = a;
            }
        if (d_cp) {   // c_j = -sum_i R_ij t_i
            for (int i = 0; i < 3; i++) {
                double gt = 0.0;
                for (int j = 0; j < 3; j++) { G[4 * i + j] += -M[4 * i + 3] * (double)d_cp[j]; gt += -M[4 * i + j] * (double)d_cp[j]; }
                G[4 * i + 3] += gt;
            }
        }
        pose_grad_and_adam(d, Bp, G, delta, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, s_M, s_g);
    }
    if (threadIdx.x != 0) return;
    se3_exp_times(d, Bp, M);
    double V[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) V[4 * i + j] = j < 3 ? M[4 * j + i] : (i == 3 ? 1.0 : 0.0);   // V = [M; 0 0 0 1]^T
    for (int q = 0; q < 16; q++) vm[q] = (float)V[q];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double a = 0.0;
            for (int k = 0; k < 4; k++) a += V[4 * i + k] * Pt[4 * k + j];
            pm[4 * i + j] = (float)a;
        }
    for (int j = 0; j < 3; j++) cp[j] = (float)(-(M[j] * M[3] + M[4 + j] * M[7] + M[8 + j] * M[11]));
}

}  // namespace gsr

extern "C" int gsr_pose_step_camera(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_viewmatrix16, const float* d_projmatrix16,
                                    const float* d_campos3, const float* projection_T16, const float* base12, float* viewmatrix16,
                                    float* projmatrix16, float* campos3, float lr, float beta1, float beta2, float eps, int64_t step, void* stream)
{
    if (!delta6 || !projection_T16 || !viewmatrix16 || !projmatrix16 || !campos3 || step < 0) return GSR_ERR_ARG;
    if (step > 0 && (!exp_avg6 || !exp_avg_sq6 || (!d_viewmatrix16 && !d_projmatrix16 && !d_campos3))) return GSR_ERR_ARG;
    const float bc1 = step > 0 ? (float)(1.0 - pow((double)beta1, (double)step)) : 1.f;
    const float bc2s = step > 0 ? (float)sqrt(1.0 - pow((double)beta2, (double)step)) : 1.f;
    hipLaunchKernelGGL(gsr::k_pose_adam_camera, dim3(1), dim3(64), 0, (hipStream_t)stream, delta6, exp_avg6, exp_avg_sq6, d_viewmatrix16,
                       d_projmatrix16, d_campos3, projection_T16, base12, viewmatrix16, projmatrix16, campos3, lr, beta1, beta2, eps, bc1, bc2s,
                       step > 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}


// ---- measurement hook: the practical HBM ceiling of the box -------------------------------------------------------------------
// A float4 streaming copy (read + write), what bench.py reports as roofline.peak_measured next to the 8 TB/s vendor peak.
// variant 0: plain 16-byte loads / stores, grid-stride; 1: the same with the nt bit; 2: four independent 16-byte loads in flight
// per lane before the first store (nt): the form the per-Gaussian backward's moment streams use; 3 (round 5): persistent workgroups,
// contiguous runs, eight loads in flight per lane -- what the chip's memory system delivers to a kernel that asks for it this way
// (tools/overlap_persist.py: 6.4-6.8 TB/s with six streams), and the honest ceiling for `frac_of_measured`.
namespace gsr {
template <int VARIANT>
__global__ __launch_bounds__(256) void k_stream_copy(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * 256u;
    size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (VARIANT == 2) {
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const float4 a = nt_load4(src + i), b = nt_load4(src + i + stride), c = nt_load4(src + i + 2 * stride), d = nt_load4(src + i + 3 * stride);
            nt_store4(dst + i, a); nt_store4(dst + i + stride, b); nt_store4(dst + i + 2 * stride, c); nt_store4(dst + i + 3 * stride, d);
        }
    }
    if (VARIANT == 3) {   // a few persistent workgroups, each with a contiguous run of 256 x 8 pieces per turn and eight loads in flight per lane
        constexpr int U = 8;
        const size_t turn = (size_t)gridDim.x * 256u * U;
        for (size_t q0 = (size_t)blockIdx.x * 256u * U + threadIdx.x; q0 < n4; q0 += turn) {
            float4 x[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const size_t q = q0 + (size_t)u * 256u; if (q < n4) x[u] = nt_load4(src + q); }
#pragma unroll
            for (int u = 0; u < U; u++) { const size_t q = q0 + (size_t)u * 256u; if (q < n4) nt_store4(dst + q, x[u]); }
        }
        return;
    }
    for (; i < n4; i += stride) {
        if (VARIANT == 0) dst[i] = src[i];
        else nt_store4(dst + i, nt_load4(src + i));
    }
}
}  // namespace gsr

extern "C" int gsr_stream_copy(const void* src, void* dst, size_t bytes, int variant, int blocks, void* stream)
{
    if (!src || !dst || (bytes & 15) || (((uintptr_t)src | (uintptr_t)dst) & 15) || blocks <= 0) return GSR_ERR_ARG;
    const size_t n4 = bytes / 16;
    const float4* s = static_cast<const float4*>(src);
    float4* d = static_cast<float4*>(dst);
    hipStream_t st = (hipStream_t)stream;
    if (variant == 0) hipLaunchKernelGGL(gsr::k_stream_copy<0>, dim3(blocks), dim3(256), 0, st, s, d, n4);
    else if (variant == 1) hipLaunchKernelGGL(gsr::k_stream_copy<1>, dim3(blocks), dim3(256), 0, st, s, d, n4);
    else if (variant == 2) hipLaunchKernelGGL(gsr::k_stream_copy<2>, dim3(blocks), dim3(256), 0, st, s, d, n4);
    else if (variant == 3) hipLaunchKernelGGL(gsr::k_stream_copy<3>, dim3(blocks), dim3(256), 0, st, s, d, n4);
    else return GSR_ERR_ARG;
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}


// ---- the trainer's per-iteration bookkeeping as three one-launch kernels (round 4; gsr_autopatch) ----------------------------------
// Between backward() and optimizer.step() the reference's train step (trainer/ht3dgs_trainer.py:137-148) evaluates, under
// no_grad, the training PSNR (utils/image_utils.py:16-18: ~10 small torch kernels), the running maximum of the visible Gaussians'
// screen radii (three boolean-mask index operations) and the densification statistics (scene/gaussian_model_ht.py:718-721: three
// more).  On models of stage A's size the iteration is bound by the host's launch path, so those ~25 launches are a third of it.
namespace gsr {
__global__ __launch_bounds__(256) void k_masked_max(float* __restrict__ dst, const int32_t* __restrict__ src, const uint8_t* __restrict__ mask, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && mask[i]) dst[i] = fmaxf(dst[i], (float)src[i]);
}

__global__ __launch_bounds__(256) void k_densify_stats_add(float* __restrict__ accum, float* __restrict__ denom, const float* __restrict__ grad3,
                                                           const uint8_t* __restrict__ mask, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && mask[i]) {
        const float gx = grad3[3 * (size_t)i], gy = grad3[3 * (size_t)i + 1];
        accum[i] += sqrtf(gx * gx + gy * gy);
        denom[i] += 1.f;
    }
}

// per channel: sum of squared differences over P pixels (partials per block), then 20 log10(1 / sqrt(mse)) by one small block
__global__ __launch_bounds__(256) void k_psnr_partial(const float* __restrict__ a, const float* __restrict__ b, int C, long long P,
                                                      float* __restrict__ partial /*[blocks][C]*/)
{
    __shared__ float s_red[4];
    const int tid = threadIdx.x;
    for (int c = 0; c < C; c++) {
        float acc = 0.f;
        const float* pa = a + (size_t)c * P;
        const float* pb = b + (size_t)c * P;
        for (long long i = (long long)blockIdx.x * 256 + tid; i < P; i += (long long)gridDim.x * 256) { const float d = pa[i] - pb[i]; acc = fmaf(d, d, acc); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if ((tid & 63) == 0) s_red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) partial[(size_t)blockIdx.x * C + c] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_psnr_finish(const float* __restrict__ partial, int blocks, int C, long long P, float* __restrict__ out)
{
    for (int c = threadIdx.x; c < C; c += 64) {
        double sse = 0.0;
        for (int k = 0; k < blocks; k++) sse += (double)partial[(size_t)k * C + c];
        const float mse = (float)(sse / (double)P);
        out[c] = 20.f * log10f(1.0f / sqrtf(mse));
    }
}

// ---- the per-model exit decision of a launch chain (gsr_batch_retire, include/gsr.h): MSE of clamp(render, 0, 1) against the target per
// image, in float64, then the retire rule.  Two launches in the manner of k_psnr_partial / k_psnr_finish, but per image (blockIdx.y) and with
// every sum in a fixed order: lane `t` of block `k` of an image adds the quads k * 256 + t, + kRetireBlocks * 256, ... of THAT image in index
// order, the lanes of a wave are folded by a xor butterfly, the four waves and then the blocks in index order.  Nothing depends on where the
// image lies in the stack: an image whose first element is not 16-byte aligned (C H W no multiple of 4) reads the same quads with four
// scalar loads instead of one float4.
constexpr int kRetireBlocks = 64;   // blocks per image (a fixed grid: the order of the sums is part of the result)

__device__ __forceinline__ double retire_sq(float x, float y)
{
#pragma clang fp contract(off)
    const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);   // clamp(render, 0, 1); a NaN stays a NaN
    const double d = (double)c - (double)y;
    return d * d;
}

__global__ __launch_bounds__(256) void k_retire_partial(const float* __restrict__ render, const float* __restrict__ target, long long n,
                                                        double* __restrict__ partial /*[B][kRetireBlocks]*/)
{
#pragma clang fp contract(off)
    __shared__ double s_red[4];
    const int tid = threadIdx.x;
    const float* a = render + (size_t)blockIdx.y * (size_t)n;
    const float* b = target + (size_t)blockIdx.y * (size_t)n;
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;   // block-uniform
    const long long quads = n >> 2;
    double acc = 0.0;
    for (long long q = (long long)blockIdx.x * 256 + tid; q < quads; q += (long long)kRetireBlocks * 256) {
        float4 x, y;
        if (vec) { x = reinterpret_cast<const float4*>(a)[q]; y = reinterpret_cast<const float4*>(b)[q]; }
        else {
            x = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
            y = make_float4(b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]);
        }
        acc += retire_sq(x.x, y.x); acc += retire_sq(x.y, y.y); acc += retire_sq(x.z, y.z); acc += retire_sq(x.w, y.w);
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) acc += retire_sq(a[4 * quads + tid], b[4 * quads + tid]);   // the last one to three elements
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[(size_t)blockIdx.y * kRetireBlocks + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(64) void k_retire_finish(const double* __restrict__ partial, int B, long long n, double mse_bar, long long exit_after,
                                                      long long step, int32_t* retired_at, double* __restrict__ mse_out)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double sse = 0.0;
    for (int k = 0; k < kRetireBlocks; k++) sse += partial[(size_t)b * kRetireBlocks + k];
    const double mse = sse / (double)n;
    mse_out[b] = mse;
    if (retired_at[b] == 0 && step > exit_after && mse < mse_bar) retired_at[b] = (int32_t)step;   // sticky; strict; NaN never passes
}
}  // namespace gsr

extern "C" int gsr_masked_max(float* dst, const int32_t* src, const uint8_t* mask, int32_t n, void* stream)
{
    if (n <= 0) return GSR_OK;
    if (!dst || !src || !mask) return GSR_ERR_ARG;
    hipLaunchKernelGGL(gsr::k_masked_max, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dst, src, mask, n);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

extern "C" int gsr_densify_stats_add(float* xyz_gradient_accum, float* denom, const float* viewspace_grad3, const uint8_t* mask, int32_t n, void* stream)
{
    if (n <= 0) return GSR_OK;
    if (!xyz_gradient_accum || !denom || !viewspace_grad3 || !mask) return GSR_ERR_ARG;
    hipLaunchKernelGGL(gsr::k_densify_stats_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyz_gradient_accum, denom, viewspace_grad3, mask, n);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

extern "C" size_t gsr_psnr_scratch_bytes(int32_t C) { return (size_t)256 * (size_t)(C > 0 ? C : 1) * sizeof(float); }

extern "C" int gsr_psnr(const float* a, const float* b, int32_t C, int64_t P, float* out, void* scratch, void* stream)
{
    if (!a || !b || !out || !scratch || C <= 0 || P <= 0) return GSR_ERR_ARG;
    const int blocks = (int)std::min<int64_t>(256, (P + 255) / 256);
    hipLaunchKernelGGL(gsr::k_psnr_partial, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, C, (long long)P, static_cast<float*>(scratch));
    hipLaunchKernelGGL(gsr::k_psnr_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<const float*>(scratch), blocks, C, (long long)P, out);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

extern "C" size_t gsr_batch_retire_scratch_bytes(int32_t B) { return (size_t)(B > 0 ? B : 1) * gsr::kRetireBlocks * sizeof(double); }

extern "C" int gsr_batch_retire(const float* render, const float* target, int32_t B, int32_t C, int32_t H, int32_t W, double mse_bar, int64_t exit_after,
                                int64_t step, int32_t* retired_at, double* mse_out, void* scratch, void* stream)
{
    if (!render || !target || !retired_at || !mse_out || !scratch || B < 1 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || step < 1 ||
        step > 0x7fffffffll || exit_after < 0 || (((uintptr_t)mse_out | (uintptr_t)scratch) & 7) != 0)
        return GSR_ERR_ARG;
    const long long n = (long long)C * H * W;
    hipLaunchKernelGGL(gsr::k_retire_partial, dim3(gsr::kRetireBlocks, B), dim3(256), 0, (hipStream_t)stream, render, target, n, static_cast<double*>(scratch));
    hipLaunchKernelGGL(gsr::k_retire_finish, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, static_cast<const double*>(scratch), (int)B, n, mse_bar,
                       (long long)exit_after, (long long)step, retired_at, mse_out);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}
