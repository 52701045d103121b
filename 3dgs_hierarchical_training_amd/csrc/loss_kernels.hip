// loss_kernels.hip -- fused photometric loss (1-l)*L1 + l*(1-SSIM) on a [3,H,W] render, forward + backward.
//
// "Next" row f-3 of SURVEY.md section 8: the reference computes this loss with five 11x11 depthwise
// convolutions per call in torch (/root/reference/trainer/losses.py:98-136 Loss.forward, :147-209 gaussian /
// create_window / _ssim; lambda_dssim = 0.2 /root/reference/arguments/__init__.py:134), on the clamped render
// (scene/gaussian_model_ht.py:883).  On MI355X those generic convolutions were 39% of the train step
// (profiles/r01_a_bench_kernel_stats.md).  Here one kernel stages a 26x26 halo tile of render and target in
// LDS, runs the separable 11-tap Gaussian for the five moments, evaluates SSIM and its three partial-derivative
// maps, and reduces L1 and SSIM sums; the backward convolves the derivative maps once more (the window is
// symmetric and zero-padded, so the adjoint is the same convolution).  clamp(0,1) of the render is fused in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gsr.h"

namespace gsr {

constexpr int kLB = 16;           // granularity of the workspace sizing (gsr_loss_workspace_bytes: an upper bound of the blocks)
constexpr int kHalo = 5;          // window 11
constexpr int kTW = 32;           // output tile of one 256-thread workgroup: 32 x (8 RP), RP = output rows per thread in the column pass
constexpr int kIW = kTW + 2 * kHalo;   // 42 staged input columns
#ifndef GSR_LOSS_RP
#define GSR_LOSS_RP 2
#endif
constexpr int kRP = GSR_LOSS_RP, kTH = 8 * kRP, kIH = kTH + 2 * kHalo;
constexpr int kLoadRounds = (kIW * kIH + 255) / 256;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

// exp(-(i-5)^2 / (2*1.5^2)) normalised, i = 0..10 (losses.py:147-150)
__device__ __constant__ float kGauss[11] = {0.0010283801f, 0.0075987581f, 0.0360007721f, 0.1093606895f, 0.2130055377f,
                                            0.2660117249f, 0.2130055377f, 0.1093606895f, 0.0360007721f, 0.0075987581f,
                                            0.0010283801f};

// clamp(v, 0, 1) as torch's: a NaN stays a NaN (fminf / fmaxf would return the other operand, and a diverged render would report
// a finite loss); +-Inf go to the bounds
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// Two moments per register pair: (x, y) and (x^2, y^2) ride through the separable window as float2, so a tap is one
// v_pk_fma_f32 instead of two fmas (per-component fma: same rounding as scalar code).
typedef float lf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lf2 lfma2(float w, lf2 v, lf2 acc) { return __builtin_elementwise_fma(lf2{w, w}, v, acc); }

// LDS row strides in 4-byte words, all = 4 (mod 32): consecutive lanes work on consecutive ROWS with 16-byte accesses, so
// eight lanes tile the 32 banks exactly (and every 4-column group stays 16-byte aligned)
constexpr int kStrIn2 = 100;      // rows of (x, y) pairs: 42 pairs = 84 words
constexpr int kStrIn1 = 68;       // rows of 42 scalars
constexpr int kStrH2 = 68;        // rows of 32 row-filtered pairs = 64 words
constexpr int kStrH1 = 36;        // rows of 32 row-filtered scalars

// Which tile a workgroup takes.  The hardware deals workgroups to the eight XCDs round-robin in launch order, so with tile = launch
// index every XCD's L2 sees every eighth tile of the frame and fetches each tile's 5-pixel halo for itself (counted: 2.1 x the
// image through the fabric).  Here XCD x takes the x-th contiguous eighth of the (channel, row, column) order instead: a tile's
// neighbours left and right and in the rows above and below run on the same L2.  GSR_LOSS_XCD_MAP=0: tile = launch index.
#ifndef GSR_LOSS_XCD_MAP
#define GSR_LOSS_XCD_MAP 1
#endif
struct LossTile { int bx, by, c; };
__device__ __forceinline__ LossTile loss_tile()
{
#if GSR_LOSS_XCD_MAP
    const uint32_t gx = gridDim.x, gy = gridDim.y, n = gx * gy * gridDim.z;
    const uint32_t lin = (blockIdx.z * gy + blockIdx.y) * gx + blockIdx.x;
    const uint32_t q = n >> 3, r = n & 7u, x = lin & 7u, k = lin >> 3;
    const uint32_t t = (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + k;
    const uint32_t row = t / gx;
    return LossTile{(int)(t - row * gx), (int)(row % gy), (int)(row / gy)};
#else
    return LossTile{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
#endif
}

// Both kernels are bound by VALU issue (a few hundred instructions per pixel, next to 40 bytes of traffic), so what is
// minimised is instructions per output: 32x32 tiles (1.7 staged inputs per output instead of 2.6 at 16x16) and a sliding
// window -- a thread produces FOUR adjacent outputs of a filter pass from 14 inputs it loads once (3.5 LDS reads per
// output instead of 11), and squares / products are formed once per input instead of once per tap.  Every output is still
// the same chain acc = fma(w[k], v[k], acc), k = 0..10, as the 16x16 kernels of round 1 computed.
// Measured at 3 x 545 x 980 (rocprofv3, tools/loss_ab.sh): forward 27.3 -> 21.4 us, backward 23.4 -> 17.2 us with 32x16 tiles
// (RP = 2; 32x32 tiles, RP = 4: 21.5 / 18.4 us -- fewer instructions but 3 instead of 5 workgroups per CU).  Issuing all of a
// thread's global loads before its first LDS store was worth as much as the instruction count (27.5 -> 21.4 us).
// grid (ceil(W/32), ceil(H/32), C); block 256.  maps: [3][C][H][W] = dS/dmu_x, dS/dE[x^2], dS/dE[xy]
__global__ __launch_bounds__(256) void k_loss_fwd(const float* __restrict__ raw, const float* __restrict__ gt, int H, int W,
                                                  int do_clamp, float* __restrict__ maps, float* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float s_in[kIH * kStrIn2];   // (x, y) pairs
    __shared__ __attribute__((aligned(16))) float s_hA[kIH * kStrH2];    // row-filtered (x, y)
    __shared__ __attribute__((aligned(16))) float s_hB[kIH * kStrH2];    // row-filtered (x^2, y^2)
    __shared__ __attribute__((aligned(16))) float s_hC[kIH * kStrH1];    // row-filtered x y
    __shared__ float s_red[2][4];
    const int tid = threadIdx.x;
    const LossTile lt = loss_tile();
    const int c = lt.c;
    const size_t P = (size_t)H * W;
    const float* x = raw + (size_t)c * P;
    const float* y = gt + (size_t)c * P;
    const int ox = lt.bx * kTW - kHalo, oy = lt.by * kTH - kHalo;
    {   // all loads of the thread are issued before the first LDS store (their latency is paid once, not per round)
        float xv[kLoadRounds], yv[kLoadRounds];
#pragma unroll
        for (int q = 0; q < kLoadRounds; q++) {
            const int i = tid + 256 * q, iy = i / kIW, ix = i - iy * kIW;
            const int gy = oy + iy, gx = ox + ix;
            const bool in = i < kIW * kIH && gx >= 0 && gx < W && gy >= 0 && gy < H;
            const size_t o = in ? (size_t)gy * W + gx : 0;
            xv[q] = in ? x[o] : 0.f; yv[q] = in ? y[o] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kLoadRounds; q++) {
            const int i = tid + 256 * q, iy = i / kIW, ix = i - iy * kIW;
            if (i < kIW * kIH) *reinterpret_cast<lf2*>(&s_in[iy * kStrIn2 + 2 * ix]) = lf2{do_clamp ? clamp01(xv[q]) : xv[q], yv[q]};
        }
    }
    __syncthreads();
    // row pass: task = (row r, group g of 4 output columns); lanes run over rows
    for (int t = tid; t < kIH * (kTW / 4); t += 256) {
        const int g = t / kIH, r = t - g * kIH;
        lf2 v[14];
        const float4* src = reinterpret_cast<const float4*>(&s_in[r * kStrIn2 + 8 * g]);
#pragma unroll
        for (int q = 0; q < 7; q++) {
            const float4 f = src[q];
            v[2 * q] = lf2{f.x, f.y}; v[2 * q + 1] = lf2{f.z, f.w};
        }
        lf2 sq[14];
        float xy[14];
#pragma unroll
        for (int k = 0; k < 14; k++) { sq[k] = v[k] * v[k]; xy[k] = v[k].x * v[k].y; }
        lf2 hA[4], hB[4];
        float hC[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            hA[i] = lf2{0.f, 0.f}; hB[i] = lf2{0.f, 0.f}; hC[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = kGauss[k];
                hA[i] = lfma2(w, v[i + k], hA[i]); hB[i] = lfma2(w, sq[i + k], hB[i]); hC[i] = fmaf(w, xy[i + k], hC[i]);
            }
        }
        float4* dA = reinterpret_cast<float4*>(&s_hA[r * kStrH2 + 8 * g]);
        float4* dB = reinterpret_cast<float4*>(&s_hB[r * kStrH2 + 8 * g]);
        dA[0] = make_float4(hA[0].x, hA[0].y, hA[1].x, hA[1].y); dA[1] = make_float4(hA[2].x, hA[2].y, hA[3].x, hA[3].y);
        dB[0] = make_float4(hB[0].x, hB[0].y, hB[1].x, hB[1].y); dB[1] = make_float4(hB[2].x, hB[2].y, hB[3].x, hB[3].y);
        *reinterpret_cast<float4*>(&s_hC[r * kStrH1 + 4 * g]) = make_float4(hC[0], hC[1], hC[2], hC[3]);
    }
    __syncthreads();
    // column pass: thread = (column cc, group of kRP output rows); lanes run over columns
    const int cc = tid & (kTW - 1), r0 = (tid / kTW) * kRP;
    lf2 mA[kRP], mB[kRP];
    float mC[kRP];
#pragma unroll
    for (int i = 0; i < kRP; i++) { mA[i] = lf2{0.f, 0.f}; mB[i] = lf2{0.f, 0.f}; mC[i] = 0.f; }
    {
        lf2 a[kRP + 10], b[kRP + 10];
        float d[kRP + 10];
#pragma unroll
        for (int k = 0; k < kRP + 10; k++) {
            a[k] = *reinterpret_cast<const lf2*>(&s_hA[(r0 + k) * kStrH2 + 2 * cc]);
            b[k] = *reinterpret_cast<const lf2*>(&s_hB[(r0 + k) * kStrH2 + 2 * cc]);
            d[k] = s_hC[(r0 + k) * kStrH1 + cc];
        }
#pragma unroll
        for (int i = 0; i < kRP; i++)
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = kGauss[k];
                mA[i] = lfma2(w, a[i + k], mA[i]); mB[i] = lfma2(w, b[i + k], mB[i]); mC[i] = fmaf(w, d[i + k], mC[i]);
            }
    }
    const int gx = lt.bx * kTW + cc;
    const size_t CP = (size_t)gridDim.z * P;
    float ssim = 0.f, l1 = 0.f;
#pragma unroll
    for (int i = 0; i < kRP; i++) {
        const int gy = lt.by * kTH + r0 + i;
        if (gx < W && gy < H) {
            const float mu1 = mA[i].x, mu2 = mA[i].y, e11 = mB[i].x, e22 = mB[i].y, e12 = mC[i];
            const float s11 = e11 - mu1 * mu1, s22 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
            const float A = 2.f * mu1 * mu2 + kC1, B = 2.f * s12 + kC2;
            const float Cc = mu1 * mu1 + mu2 * mu2 + kC1, D = s11 + s22 + kC2;
            const float iCD = 1.f / (Cc * D);
            const float sv = A * B * iCD;
            ssim += sv;
            // partial derivatives of S w.r.t. the three moments that depend on x (mu_x, E[x^2], E[xy])
            const float dS_dmu = 2.f * mu2 * (B - A) * iCD - 2.f * mu1 * sv / Cc + 2.f * mu1 * sv / D;
            const float dS_de11 = -sv / D;
            const float dS_de12 = 2.f * A * iCD;
            const size_t pid = (size_t)c * P + (size_t)gy * W + gx;
            maps[pid] = dS_dmu; maps[CP + pid] = dS_de11; maps[2 * CP + pid] = dS_de12;
            const lf2 ctr = *reinterpret_cast<const lf2*>(&s_in[(r0 + i + kHalo) * kStrIn2 + 2 * (cc + kHalo)]);
            l1 += fabsf(ctr.x - ctr.y);
        }
    }
    // block reduction (wave shuffles, then 4 partials)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ssim += __shfl_xor(ssim, off, 64); l1 += __shfl_xor(l1, off, 64); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = ssim; s_red[1][tid >> 6] = l1; }
    __syncthreads();
    if (tid == 0) {
        const size_t b = ((size_t)lt.c * gridDim.y + lt.by) * gridDim.x + lt.bx;   // the TILE's slot: the finishing sum does not see the map
        partial[2 * b] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        partial[2 * b + 1] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    }
}

// single block: deterministic reduction of the per-block partials -> out[0] = loss, out[1] = mean ssim, out[2] = mean l1
// images > 1 (a stack of independent images, gsr_loss_forward_batched): inv_count is ONE image's 1 / (C H W), so the two sums are
// sums of per-image means; out[0] = the SUM of the images' losses, out[1] / out[2] their mean SSIM / mean L1
__global__ __launch_bounds__(1024) void k_loss_finish(const float* __restrict__ partial, int nblocks, float inv_count, float lambda,
                                                      float* __restrict__ out, int images, int nout = 3, float* __restrict__ loss_dup = nullptr)
{
    __shared__ double s0[1024], s1[1024];
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nblocks; i += 1024) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    s0[threadIdx.x] = a; s1[threadIdx.x] = b;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (threadIdx.x < off) { s0[threadIdx.x] += s0[threadIdx.x + off]; s1[threadIdx.x] += s1[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ms = s0[0] * inv_count, ml = s1[0] * inv_count;
        out[0] = (float)((1.0 - lambda) * ml + lambda * ((double)images - ms));
        out[1] = (float)(ms / images); out[2] = (float)(ml / images);
        if (nout >= 6) {   // what Loss.forward reports beside the loss (/root/reference/trainer/losses.py:128-136), so the caller needs no torch ops for them
            out[3] = (float)((1.0 - lambda) * (ml / images));    // loss_rgb = (1 - lambda) * mean L1
            out[4] = (float)(1.0 - ms / images);                 // loss_dssim = 1 - mean SSIM
            out[5] = 0.f;                                        // loss_depth when no depth term is configured
        }
        if (loss_dup) *loss_dup = out[0];
    }
}

__global__ __launch_bounds__(256) void k_loss_bwd(const float* __restrict__ raw, const float* __restrict__ gt, int H, int W,
                                                  int do_clamp, const float* __restrict__ maps, const float* __restrict__ gscale,
                                                  float inv_count, float lambda, float* __restrict__ d_raw)
{
    __shared__ __attribute__((aligned(16))) float s_mA[kIH * kStrIn2];   // (dS/dmu_x, dS/dE[x^2])
    __shared__ __attribute__((aligned(16))) float s_mC[kIH * kStrIn1];   // dS/dE[xy]
    __shared__ __attribute__((aligned(16))) float s_hA[kIH * kStrH2];
    __shared__ __attribute__((aligned(16))) float s_hC[kIH * kStrH1];
    const int tid = threadIdx.x;
    const LossTile lt = loss_tile();
    const int c = lt.c;
    const size_t P = (size_t)H * W, CP = (size_t)gridDim.z * P;
    const int ox = lt.bx * kTW - kHalo, oy = lt.by * kTH - kHalo;
    {
        float a[kLoadRounds], bb[kLoadRounds], d[kLoadRounds];
#pragma unroll
        for (int q = 0; q < kLoadRounds; q++) {
            const int i = tid + 256 * q, iy = i / kIW, ix = i - iy * kIW;
            const int gy = oy + iy, gx = ox + ix;
            const bool in = i < kIW * kIH && gx >= 0 && gx < W && gy >= 0 && gy < H;
            const size_t pid = in ? (size_t)c * P + (size_t)gy * W + gx : 0;
            a[q] = in ? maps[pid] : 0.f; bb[q] = in ? maps[CP + pid] : 0.f; d[q] = in ? maps[2 * CP + pid] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kLoadRounds; q++) {
            const int i = tid + 256 * q, iy = i / kIW, ix = i - iy * kIW;
            if (i < kIW * kIH) {
                *reinterpret_cast<lf2*>(&s_mA[iy * kStrIn2 + 2 * ix]) = lf2{a[q], bb[q]};
                s_mC[iy * kStrIn1 + ix] = d[q];
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < kIH * (kTW / 4); t += 256) {
        const int g = t / kIH, r = t - g * kIH;
        lf2 v[14];
        float d[16];
        const float4* srcA = reinterpret_cast<const float4*>(&s_mA[r * kStrIn2 + 8 * g]);
        const float4* srcC = reinterpret_cast<const float4*>(&s_mC[r * kStrIn1 + 4 * g]);
#pragma unroll
        for (int q = 0; q < 7; q++) {
            const float4 f = srcA[q];
            v[2 * q] = lf2{f.x, f.y}; v[2 * q + 1] = lf2{f.z, f.w};
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {   // 16 scalars: the last two lie in the row's padding (stride 68 >= 4 * 7 + 16)
            const float4 f = srcC[q];
            d[4 * q] = f.x; d[4 * q + 1] = f.y; d[4 * q + 2] = f.z; d[4 * q + 3] = f.w;
        }
        lf2 hA[4];
        float hC[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            hA[i] = lf2{0.f, 0.f}; hC[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = kGauss[k];
                hA[i] = lfma2(w, v[i + k], hA[i]); hC[i] = fmaf(w, d[i + k], hC[i]);
            }
        }
        float4* dA = reinterpret_cast<float4*>(&s_hA[r * kStrH2 + 8 * g]);
        dA[0] = make_float4(hA[0].x, hA[0].y, hA[1].x, hA[1].y); dA[1] = make_float4(hA[2].x, hA[2].y, hA[3].x, hA[3].y);
        *reinterpret_cast<float4*>(&s_hC[r * kStrH1 + 4 * g]) = make_float4(hC[0], hC[1], hC[2], hC[3]);
    }
    __syncthreads();
    const int cc = tid & (kTW - 1), r0 = (tid / kTW) * kRP;
    const int gx = lt.bx * kTW + cc;
    if (gx >= W) return;
    lf2 cA[kRP];
    float c2[kRP];
    {
        lf2 a[kRP + 10];
        float d[kRP + 10];
#pragma unroll
        for (int k = 0; k < kRP + 10; k++) {
            a[k] = *reinterpret_cast<const lf2*>(&s_hA[(r0 + k) * kStrH2 + 2 * cc]);
            d[k] = s_hC[(r0 + k) * kStrH1 + cc];
        }
#pragma unroll
        for (int i = 0; i < kRP; i++) {
            cA[i] = lf2{0.f, 0.f}; c2[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = kGauss[k];
                cA[i] = lfma2(w, a[i + k], cA[i]); c2[i] = fmaf(w, d[i + k], c2[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kRP; i++) {
        const int gy = lt.by * kTH + r0 + i;
        if (gy >= H) break;
        const size_t pid = (size_t)c * P + (size_t)gy * W + gx;
        const float r = raw[pid], yv = gt[pid];
        const float xv = do_clamp ? clamp01(r) : r;
        const float dssim = cA[i].x + 2.f * xv * cA[i].y + yv * c2[i];   // d(sum of SSIM map)/dx
        const float diff = xv - yv;
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        float g = ((1.f - lambda) * sgn - lambda * dssim) * inv_count;
        if (do_clamp && (r < 0.f || r > 1.f)) g = 0.f;               // clamp backward (inclusive pass-through like torch)
        d_raw[pid] = g * (gscale ? gscale[0] : 1.f);
    }
}

// ---- depth term of Loss.forward (/root/reference/trainer/losses.py:86-95, :114-119; the MiDaS scale-and-shift-invariant loss
// :259-393 constructed with alpha = 0.5, scales = 1, :41) ----------------------------------------------------------------------
// p = the rasterizer's depth plane, g = depth_gt, pc = min(max(p, lo), hi) (the two masked assignments of :116-117, fused).
//   'l1' (kind 0):        sum |pc - g| / (H W)
//   'invariant' (kind 1): m = g > 0.02; (s, t) = the masked least-squares fit of s pc + t to g; d = m (s pc + t - g);
//                         data = sum d^2 / (2 M), reg = sum over adjacent pairs m_a m_b |d_b - d_a| / M, loss = data + 0.5 reg
// The chain is launch-bound (five passes over one or two planes of a few MB), so it is four short launches forward and one
// backward.  Every sum is float64 with a fixed grid and fixed-order partials -- no atomics, the same bits on every run; det = a00 a11 -
// a01^2 is a difference of products of sums and cancels in binary32.  The residual d is evaluated by ONE function (depth_resid) in
// the forward and the backward, so the sign of a pair's |.| is decided identically in both.
constexpr int kDS1 = 256;          // workgroups of k_depth_sums at most (one partial row per thread of the consumers)
constexpr int kDS2 = 1024;         // workgroups of k_depth_terms at most
constexpr int kDV = 5;             // values per partial row
constexpr int kDepthImagesMax = 65535;   // images of a stack: one grid row each
constexpr float kDepthValid = 0.02f;   // mask = depth_gt > 0.02 (losses.py:92; a constant of the reference, not the clamp bound)
// workspace: coefficients | partial rows of k_depth_sums | partial rows of k_depth_terms
enum { kDcS = 0, kDcT, kDcInvM, kDcU0, kDcU1, kDcLs, kDcLt, kDcLoss, kDcSums /* 5 */, kDcDet = kDcSums + kDV, kDcLambda, kDcN = 16 };
struct DepthWs { double coef[kDcN]; double p1[kDS1 * kDV]; double p2[kDS2 * kDV]; };

__device__ __forceinline__ float depth_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ double depth_resid(double s, double t, float pr, float gr, float lo, float hi)
{
    return __builtin_fma(s, (double)depth_clamp(pr, lo, hi), t) - (double)gr;
}
__device__ __forceinline__ double depth_sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// sum of the workgroup's kDV lane values -> dst[0..kDV) (thread 0 writes; wave shuffles, then the four waves in index order)
__device__ __forceinline__ void depth_block_sum(double (&v)[kDV], double* s_red, double* __restrict__ dst)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kDV; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < kDV; k++) s_red[(tid >> 6) * kDV + k] = v[k];
    __syncthreads();
    if (tid == 0)
#pragma unroll
        for (int k = 0; k < kDV; k++) dst[k] = ((s_red[k] + s_red[kDV + k]) + s_red[2 * kDV + k]) + s_red[3 * kDV + k];
}

// column sums of n <= NT partial rows, the same tree in every workgroup that calls it (every thread of the workgroup calls)
template <int NT>
__device__ __forceinline__ void depth_rows_sum(const double* __restrict__ rows, int n, double* s_buf, double (&out)[kDV])
{
    const int r = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kDV; k++) s_buf[k * NT + r] = r < n ? rows[r * kDV + k] : 0.0;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (r < off)
#pragma unroll
            for (int k = 0; k < kDV; k++) s_buf[k * NT + r] += s_buf[k * NT + r + off];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kDV; k++) out[k] = s_buf[k * NT];
    __syncthreads();
}

// pass 1: the five sums of the normal equations (kind 1) or sum |pc - g| (kind 0); grid <= kDS1, one partial row per workgroup.
// blockIdx.y = the image of a stack [images,H,W] (gsr_depth_loss_*_batched): plane b at b P floats, its rows in ws[b]; nothing is
// shared between images.  vec = which elements a lane adds: 1 = four consecutive elements per lane per trip, then the scalar tail
// (what an aligned single plane has always taken), 0 = one element per lane per trip (a misaligned single plane).  The two group the
// float64 additions differently, so a stack ALWAYS walks with vec = 1 -- plane b of a stack is 16-byte aligned only when b P is a
// multiple of 4 -- and only the WIDTH of the loads follows the plane's address: an image's bits do not depend on where it lies.
__global__ __launch_bounds__(256) void k_depth_sums(const float* __restrict__ p, const float* __restrict__ g, size_t P, int vec, int kind,
                                                    float lo, float hi, DepthWs* __restrict__ ws)
{
    __shared__ double s_red[4 * kDV];
    p += (size_t)blockIdx.y * P; g += (size_t)blockIdx.y * P;
    double v[kDV] = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto acc = [&](float pr, float gr) {
        const double pc = (double)depth_clamp(pr, lo, hi), gd = (double)gr;
        if (kind == 0) v[0] += fabs(pc - gd);
        else if (gr > kDepthValid) { v[0] += pc * pc; v[1] += pc; v[2] += 1.0; v[3] += pc * gd; v[4] += gd; }
    };
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n4 = vec ? P / 4 : 0;
    const bool wide = (((uintptr_t)p | (uintptr_t)g) & 15) == 0;   // (uniform over the workgroup)
    for (size_t i = first; i < n4; i += stride) {
        float4 a, b;
        if (wide) { a = reinterpret_cast<const float4*>(p)[i]; b = reinterpret_cast<const float4*>(g)[i]; }   // 16-byte loads
        else { a = make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]); b = make_float4(g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]); }
        acc(a.x, b.x); acc(a.y, b.y); acc(a.z, b.z); acc(a.w, b.w);
    }
    for (size_t i = n4 * 4 + first; i < P; i += stride) acc(p[i], g[i]);
    depth_block_sum(v, s_red, ws[blockIdx.y].p1 + (size_t)blockIdx.x * kDV);
}

// pass 2 (kind 1): every workgroup reduces the partial rows in the same order and solves the 2x2 in float64 -- the same (s, t)
// everywhere -- then walks its pixels with the neighbour to the right and the one below.  Partial row: sum d^2, sum |d_b - d_a|,
// sum sgn(d_b - d_a) (pc_b - pc_a) (= M d reg / ds), sum d pc, sum d (= M d data / ds, dt; zero up to rounding at the fit).
__global__ __launch_bounds__(256) void k_depth_terms(const float* __restrict__ p, const float* __restrict__ g, int H, int W, float lo,
                                                     float hi, int n1, DepthWs* __restrict__ ws)
{
    __shared__ double s_buf[kDV * 256];
    __shared__ double s_red[4 * kDV];
    DepthWs& w = ws[blockIdx.y];            // blockIdx.y = the image of a stack: its own plane, rows, fit and coefficients
    double* __restrict__ coef = w.coef;
    double S[kDV];
    depth_rows_sum<256>(w.p1, n1, s_buf, S);
    const double det = S[0] * S[2] - S[1] * S[1];
    double s = 0.0, t = 0.0;
    if (det != 0.0) { s = (S[2] * S[3] - S[1] * S[4]) / det; t = (-S[1] * S[3] + S[0] * S[4]) / det; }   // losses.py:273-279
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        coef[kDcS] = s; coef[kDcT] = t; coef[kDcDet] = det;
#pragma unroll
        for (int k = 0; k < kDV; k++) coef[kDcSums + k] = S[k];
    }
    double v[kDV] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t P = (size_t)H * W, stride = (size_t)gridDim.x * 256;
    p += (size_t)blockIdx.y * P; g += (size_t)blockIdx.y * P;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < P; i += stride) {
        const float gi = g[i];
        if (!(gi > kDepthValid)) continue;
        const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
        const float pi = p[i];
        const double pc = (double)depth_clamp(pi, lo, hi), d = depth_resid(s, t, pi, gi, lo, hi);
        v[0] += d * d; v[3] += d * pc; v[4] += d;
        if (x + 1 < W) {
            const float gj = g[i + 1];
            if (gj > kDepthValid) {
                const float pj = p[i + 1];
                const double diff = depth_resid(s, t, pj, gj, lo, hi) - d;
                v[1] += fabs(diff); v[2] += depth_sgn(diff) * ((double)depth_clamp(pj, lo, hi) - pc);
            }
        }
        if (y + 1 < H) {
            const float gj = g[i + W];
            if (gj > kDepthValid) {
                const float pj = p[i + W];
                const double diff = depth_resid(s, t, pj, gj, lo, hi) - d;
                v[1] += fabs(diff); v[2] += depth_sgn(diff) * ((double)depth_clamp(pj, lo, hi) - pc);
            }
        }
    }
    depth_block_sum(v, s_red, w.p2 + (size_t)blockIdx.x * kDV);
}

// the stack's totals from the images' finished coefficients, one thread: *out_sum (may be NULL) = the SUM of the images' unweighted
// terms, added in float64 in index order.  terms6 (may be NULL): the six-float vector of gsr_loss_forward_terms, completed as
// k_loss_finish completes it for a stack -- the weighted SUM is added to its total, slot 5 receives the MEAN of the unweighted terms;
// loss_dup: a second place for the total.  (images == 1: sum = mean = the image's term.)
__device__ __forceinline__ void depth_total(const DepthWs* __restrict__ ws, int images, double lambda, float* __restrict__ out_sum,
                                            float* __restrict__ terms6, float* __restrict__ loss_dup)
{
    double loss = 0.0;
    for (int b = 0; b < images; b++) loss += ws[b].coef[kDcLoss];
    if (out_sum) *out_sum = (float)loss;
    if (terms6) {
        terms6[0] = (float)((double)terms6[0] + lambda * loss);
        terms6[5] = (float)(loss / (double)images);
        if (loss_dup) *loss_dup = terms6[0];
    }
}

// one workgroup per image: out6[b] = {loss_depth, s, t, M, data, reg} and the backward's coefficients.  With dL/ds = Ls, dL/dt = Lt
// and the normal matrix A = [[a00, a01], [a01, a11]]: u = A^-1 (Ls, Lt), and pixel i adds -u0 (d_i + s pc_i) - u1 s (the closed form
// of ds/dpc_i, dt/dpc_i contracted with (Ls, Lt)).  A single image (grid 1) finishes with depth_total here; a stack's totals need
// every image's term and take a launch of their own (k_depth_total).
__global__ __launch_bounds__(1024) void k_depth_finish(DepthWs* ws, int n1, int n2, int kind, double npix, double lambda,
                                                       float* __restrict__ out6, float* __restrict__ out_sum, float* __restrict__ terms6,
                                                       float* __restrict__ loss_dup)
{
    __shared__ double s_buf[kDV * 1024];
    DepthWs& w = ws[blockIdx.x];
    double* coef = w.coef;                  // (not __restrict__: depth_total below reads what is stored through it)
    out6 += 6 * (size_t)blockIdx.x;
    double T[kDV];
    depth_rows_sum<1024>(kind == 0 ? w.p1 : w.p2, kind == 0 ? n1 : n2, s_buf, T);
    if (threadIdx.x != 0) return;
    double loss = 0.0, s = 0.0, t = 0.0, M = npix, data = 0.0, reg = 0.0, invM = 0.0, u0 = 0.0, u1 = 0.0, Ls = 0.0, Lt = 0.0;
    if (kind == 0) loss = T[0] / npix;
    else {
        s = coef[kDcS]; t = coef[kDcT]; M = coef[kDcSums + 2];
        if (M > 0.0) {   // reduction_batch_based (:284-293): both terms are 0 when no pixel is valid
            invM = 1.0 / M;
            data = T[0] / (2.0 * M); reg = T[1] / M; loss = data + 0.5 * reg;
            const double det = coef[kDcDet], a00 = coef[kDcSums], a01 = coef[kDcSums + 1];
            if (det != 0.0) {   // (s = t = 0 are constants otherwise: no gradient through the fit, :270-279)
                Ls = (T[3] + 0.5 * T[2]) * invM; Lt = T[4] * invM;
                u0 = (M * Ls - a01 * Lt) / det; u1 = (-a01 * Ls + a00 * Lt) / det;
            }
        }
    }
    coef[kDcS] = s; coef[kDcT] = t; coef[kDcInvM] = kind == 0 ? 1.0 / npix : invM; coef[kDcU0] = u0; coef[kDcU1] = u1;
    coef[kDcLs] = Ls; coef[kDcLt] = Lt; coef[kDcLoss] = loss; coef[kDcLambda] = lambda;
    out6[0] = (float)loss; out6[1] = (float)s; out6[2] = (float)t; out6[3] = (float)M; out6[4] = (float)data; out6[5] = (float)reg;
    if (gridDim.x == 1) depth_total(ws, 1, lambda, out_sum, terms6, loss_dup);
}

__global__ void k_depth_total(const DepthWs* __restrict__ ws, int images, double lambda, float* __restrict__ out_sum,
                              float* __restrict__ terms6, float* __restrict__ loss_dup)
{
    if (threadIdx.x == 0) depth_total(ws, images, lambda, out_sum, terms6, loss_dup);
}

// d_p[i] = upstream * lambda * pass(p_i) * dL/dpc_i, one store per pixel.  pass: a pixel strictly outside [lo, hi] gets zero, one on a
// bound passes (the masked assignments of :116-117).  invariant: m_i [ s/M (d_i + 0.5 stencil_i) - u0 (d_i + s pc_i) - u1 s ], stencil
// = the signs of the pixel's four incident pairs.  blockIdx.y = the image of a stack, with ITS coefficients: the gradient of the SUM of
// the images' terms, i.e. every image receives exactly the gradient of its own.
__global__ __launch_bounds__(256) void k_depth_bwd(const float* __restrict__ p, const float* __restrict__ g, int H, int W, int kind, float lo,
                                                   float hi, double lambda, const DepthWs* __restrict__ ws, const float* __restrict__ gscale,
                                                   float* __restrict__ d_p)
{
    const double* __restrict__ coef = ws[blockIdx.y].coef;
    const double up = (gscale ? (double)gscale[0] : 1.0) * lambda;
    const double s = coef[kDcS], t = coef[kDcT], invM = coef[kDcInvM], u0 = coef[kDcU0], u1 = coef[kDcU1];
    const size_t P = (size_t)H * W, stride = (size_t)gridDim.x * 256;
    p += (size_t)blockIdx.y * P; g += (size_t)blockIdx.y * P; d_p += (size_t)blockIdx.y * P;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < P; i += stride) {
        const float pi = p[i], gi = g[i];
        float out = 0.f;
        if (pi >= lo && pi <= hi) {
            if (kind == 0) out = (float)(up * invM * depth_sgn((double)pi - (double)gi));
            else if (gi > kDepthValid) {
                const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
                const double d = depth_resid(s, t, pi, gi, lo, hi);
                double st = 0.0;
                if (x > 0 && g[i - 1] > kDepthValid) st += depth_sgn(d - depth_resid(s, t, p[i - 1], g[i - 1], lo, hi));
                if (x + 1 < W && g[i + 1] > kDepthValid) st -= depth_sgn(depth_resid(s, t, p[i + 1], g[i + 1], lo, hi) - d);
                if (y > 0 && g[i - W] > kDepthValid) st += depth_sgn(d - depth_resid(s, t, p[i - W], g[i - W], lo, hi));
                if (y + 1 < H && g[i + W] > kDepthValid) st -= depth_sgn(depth_resid(s, t, p[i + W], g[i + W], lo, hi) - d);
                out = (float)(up * (s * invM * (d + 0.5 * st) - u0 * (d + s * (double)pi) - u1 * s));
            }
        }
        d_p[i] = out;
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_loss_workspace_bytes(int32_t C, int32_t H, int32_t W)
{
    const size_t nb = (size_t)((W + kLB - 1) / kLB) * ((H + kLB - 1) / kLB) * C;
    const size_t maps = (size_t)3 * C * H * W * sizeof(float);
    return ((maps + 255) & ~(size_t)255) + ((nb * 2 * sizeof(float) + 255) & ~(size_t)255);
}
size_t gsr_loss_workspace_bytes_batched(int32_t images, int32_t C, int32_t H, int32_t W) { return gsr_loss_workspace_bytes(images * C, H, W); }

static int loss_forward_impl(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                             int32_t clamp01_render, void* workspace, float* out3, void* stream, int nout, float* loss_dup = nullptr);
int gsr_loss_forward_batched(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                             int32_t clamp01_render, void* workspace, float* out3, void* stream)
{
    return loss_forward_impl(render, target, images, C, H, W, lambda_dssim, clamp01_render, workspace, out3, stream, 3);
}
int gsr_loss_forward_terms(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                           int32_t clamp01_render, void* workspace, float* out6, float* loss_copy, void* stream)
{
    return loss_forward_impl(render, target, images, C, H, W, lambda_dssim, clamp01_render, workspace, out6, stream, 6, loss_copy);
}
static int loss_forward_impl(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                             int32_t clamp01_render, void* workspace, float* out3, void* stream, int nout, float* loss_dup)
{
    if (!render || !target || !workspace || !out3 || images <= 0 || C <= 0 || H <= 0 || W <= 0) return GSR_ERR_ARG;
    const int CT = images * C;   // channels are independent of one another in both terms: the stack is CT channel planes
    const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, CT), block(256);
    const size_t maps_bytes = (((size_t)3 * CT * H * W * sizeof(float)) + 255) & ~(size_t)255;
    float* maps = static_cast<float*>(workspace);
    float* partial = reinterpret_cast<float*>(static_cast<uint8_t*>(workspace) + maps_bytes);
    const int nb = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(k_loss_fwd, grid, block, 0, (hipStream_t)stream, render, target, H, W, clamp01_render, maps, partial);
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(1024), 0, (hipStream_t)stream, partial, nb, 1.0f / ((float)C * H * W), lambda_dssim, out3, images, nout, loss_dup);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_loss_backward_batched(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                              int32_t clamp01_render, const void* workspace, const float* grad_loss, float* d_render, void* stream)
{
    if (!render || !target || !workspace || !d_render || images <= 0 || C <= 0 || H <= 0 || W <= 0) return GSR_ERR_ARG;
    const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, images * C), block(256);
    // every image with ITS OWN normalisation 1 / (C H W): the gradient of the sum of the images' losses
    hipLaunchKernelGGL(k_loss_bwd, grid, block, 0, (hipStream_t)stream, render, target, H, W, clamp01_render,
                       static_cast<const float*>(workspace), grad_loss, 1.0f / ((float)C * H * W), lambda_dssim, d_render);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_loss_forward(const float* render, const float* target, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                     int32_t clamp01_render, void* workspace, float* out3, void* stream)
{
    return gsr_loss_forward_batched(render, target, 1, C, H, W, lambda_dssim, clamp01_render, workspace, out3, stream);
}

int gsr_loss_backward(const float* render, const float* target, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                      int32_t clamp01_render, const void* workspace, const float* grad_loss, float* d_render, void* stream)
{
    return gsr_loss_backward_batched(render, target, 1, C, H, W, lambda_dssim, clamp01_render, workspace, grad_loss, d_render, stream);
}

size_t gsr_depth_loss_workspace_bytes_batched(int32_t images, int32_t H, int32_t W)
{
    (void)H; (void)W;   // per image: coefficients + the two fixed grids' partial rows, the same size for every plane
    return ((size_t)std::max(images, 1) * sizeof(DepthWs) + 255) & ~(size_t)255;
}
size_t gsr_depth_loss_workspace_bytes(int32_t H, int32_t W) { return gsr_depth_loss_workspace_bytes_batched(1, H, W); }

// vec: the element-to-lane assignment of k_depth_sums.  A single plane takes the one its alignment has always selected; a stack takes
// 1 for every plane, wherever it lies.
static int depth_loss_forward_impl(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int vec, int32_t kind,
                                   float clamp_lo, float clamp_hi, float lambda_depth, void* workspace, float* out6, float* out_sum, float* terms6,
                                   float* loss_copy, void* stream)
{
    if (!depth || !depth_gt || !workspace || !out6 || images <= 0 || images > kDepthImagesMax || H <= 0 || W <= 0 ||
        (kind != GSR_DEPTH_LOSS_L1 && kind != GSR_DEPTH_LOSS_INVARIANT) || !(clamp_lo <= clamp_hi) || ((uintptr_t)workspace & 7) != 0)
        return GSR_ERR_ARG;
    DepthWs* ws = static_cast<DepthWs*>(workspace);
    const size_t P = (size_t)H * W;
    const int n1 = (int)std::min<size_t>(kDS1, (P + 1023) / 1024), n2 = (int)std::min<size_t>(kDS2, (P + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_depth_sums, dim3(n1, images), dim3(256), 0, st, depth, depth_gt, P, vec, (int)kind, clamp_lo, clamp_hi, ws);
    if (kind == GSR_DEPTH_LOSS_INVARIANT)
        hipLaunchKernelGGL(k_depth_terms, dim3(n2, images), dim3(256), 0, st, depth, depth_gt, (int)H, (int)W, clamp_lo, clamp_hi, n1, ws);
    hipLaunchKernelGGL(k_depth_finish, dim3(images), dim3(1024), 0, st, ws, n1, n2, (int)kind, (double)P, (double)lambda_depth, out6, out_sum,
                       terms6, loss_copy);
    if (images > 1 && (out_sum || terms6))
        hipLaunchKernelGGL(k_depth_total, dim3(1), dim3(64), 0, st, ws, (int)images, (double)lambda_depth, out_sum, terms6, loss_copy);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}
static int depth_plane_vec(const float* depth, const float* depth_gt) { return ((((uintptr_t)depth | (uintptr_t)depth_gt) & 15) == 0) ? 1 : 0; }

int gsr_depth_loss_forward(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                           float lambda_depth, void* workspace, float* out6, void* stream)
{
    return depth_loss_forward_impl(depth, depth_gt, 1, H, W, depth_plane_vec(depth, depth_gt), kind, clamp_lo, clamp_hi, lambda_depth, workspace, out6,
                                   nullptr, nullptr, nullptr, stream);
}

int gsr_depth_loss_forward_terms(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                                 float lambda_depth, void* workspace, float* out6, float* terms6, float* loss_copy, void* stream)
{
    if (!terms6) return GSR_ERR_ARG;
    return depth_loss_forward_impl(depth, depth_gt, 1, H, W, depth_plane_vec(depth, depth_gt), kind, clamp_lo, clamp_hi, lambda_depth, workspace, out6,
                                   nullptr, terms6, loss_copy, stream);
}

int gsr_depth_loss_forward_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind, float clamp_lo,
                                   float clamp_hi, float lambda_depth, void* workspace, float* out6, float* out_sum, void* stream)
{
    if (!out_sum) return GSR_ERR_ARG;
    return depth_loss_forward_impl(depth, depth_gt, images, H, W, 1, kind, clamp_lo, clamp_hi, lambda_depth, workspace, out6, out_sum, nullptr,
                                   nullptr, stream);
}

int gsr_depth_loss_forward_terms_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind,
                                         float clamp_lo, float clamp_hi, float lambda_depth, void* workspace, float* out6, float* terms6,
                                         float* loss_copy, void* stream)
{
    if (!terms6) return GSR_ERR_ARG;
    return depth_loss_forward_impl(depth, depth_gt, images, H, W, 1, kind, clamp_lo, clamp_hi, lambda_depth, workspace, out6, nullptr, terms6,
                                   loss_copy, stream);
}

static int depth_loss_backward_impl(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind, float clamp_lo,
                                    float clamp_hi, float lambda_depth, const void* workspace, const float* grad_loss, float* d_depth,
                                    void* stream)
{
    if (!depth || !depth_gt || !workspace || !d_depth || images <= 0 || images > kDepthImagesMax || H <= 0 || W <= 0 ||
        (kind != GSR_DEPTH_LOSS_L1 && kind != GSR_DEPTH_LOSS_INVARIANT))
        return GSR_ERR_ARG;
    const DepthWs* ws = static_cast<const DepthWs*>(workspace);
    const size_t P = (size_t)H * W;
    const int nb = (int)std::min<size_t>(2048, (P + 255) / 256);
    hipLaunchKernelGGL(k_depth_bwd, dim3(nb, images), dim3(256), 0, (hipStream_t)stream, depth, depth_gt, (int)H, (int)W, (int)kind, clamp_lo,
                       clamp_hi, (double)lambda_depth, ws, grad_loss, d_depth);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_depth_loss_backward_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind, float clamp_lo,
                                    float clamp_hi, float lambda_depth, const void* workspace, const float* grad_loss, float* d_depth,
                                    void* stream)
{
    if (((uintptr_t)workspace & 7) != 0) return GSR_ERR_ARG;
    return depth_loss_backward_impl(depth, depth_gt, images, H, W, kind, clamp_lo, clamp_hi, lambda_depth, workspace, grad_loss, d_depth, stream);
}

int gsr_depth_loss_backward(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                            float lambda_depth, const void* workspace, const float* grad_loss, float* d_depth, void* stream)
{
    return depth_loss_backward_impl(depth, depth_gt, 1, H, W, kind, clamp_lo, clamp_hi, lambda_depth, workspace, grad_loss, d_depth, stream);
}

}  // extern "C"
