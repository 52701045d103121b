// adam_math.h -- the Adam update shared by k_adam (optim_kernels.hip) and the optimizer-in-backward mode of
// k_preprocess_bwd (gsr_kernels.hip).  Update rule = torch.optim.Adam without amsgrad / weight decay, as the reference
// constructs it (/root/reference/scene/gaussian_model_ht.py:275-289):
//   m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float b1, float b2, float eps, float step_size,
                                         float inv_bc2s)
{
    m = fmaf(g - m, 1.f - b1, m);
    v = fmaf(v, b2, (1.f - b2) * g * g);
    const float denom = sqrtf(v) * inv_bc2s + eps;
    p -= step_size * (m / denom);
}

// Did the update leave a stream element exactly as it was loaded?  The in-place streams can then leave its stores out: the value is
// already in memory (a Gaussian no view has reached yet -- g = m = v = 0 -- or an SH band above the active degree: p' = p, m' = m,
// v' = v).  Decided from the computed outputs alone, word by word as integers, so it is exact whatever adam_one does: a -0.0 moment
// that comes back +0.0 counts as changed and is stored, a NaN counts as unchanged only when its bits are the same.
__device__ __forceinline__ bool adam_unchanged(float p0, float m0, float v0, float p1, float m1, float v1)
{
    return ((__float_as_uint(p0) ^ __float_as_uint(p1)) | (__float_as_uint(m0) ^ __float_as_uint(m1)) |
            (__float_as_uint(v0) ^ __float_as_uint(v1))) == 0u;
}
__device__ __forceinline__ uint32_t adam_diff4(const float4& a, const float4& b)
{
    return (__float_as_uint(a.x) ^ __float_as_uint(b.x)) | (__float_as_uint(a.y) ^ __float_as_uint(b.y)) |
           (__float_as_uint(a.z) ^ __float_as_uint(b.z)) | (__float_as_uint(a.w) ^ __float_as_uint(b.w));
}
__device__ __forceinline__ bool adam_unchanged4(const float4& p0, const float4& m0, const float4& v0, const float4& p1, const float4& m1,
                                                const float4& v1)
{
    return (adam_diff4(p0, p1) | adam_diff4(m0, m1) | adam_diff4(v0, v1)) == 0u;
}

// The stores are kept or left out by whole aligned groups of LANES consecutive lanes -- eight 16-byte elements = one 128-byte line of
// each of the three streams: a line the update changed anywhere is written in full, as before, and only a line that is unchanged
// throughout is not written at all, so no full-line write ever turns into a partial one (which the memory side would have to merge).
// `lane` = the thread's lane in its wave; lanes that are not active count as unchanged.
template <int LANES>
__device__ __forceinline__ bool adam_line_changed(bool changed, int lane)
{
    static_assert(LANES == 8 || LANES == 32, "aligned lane groups");
    const unsigned long long b = __ballot(changed);
    return ((b >> (lane & (64 - LANES))) & (LANES == 32 ? 0xffffffffull : 0xffull)) != 0ull;
}

// Streaming accesses: parameters and moments are touched once per step (1.4 kB per Gaussian), so they carry the `nt` bit and
// do not displace the splats, lists and checkpoints the neighbouring kernels keep in L2 / MALL.
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4* a)
{
    const nt_f4 r = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(a));
    return make_float4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ void nt_store4(float4* a, const float4& x)
{
    nt_f4 r = {x.x, x.y, x.z, x.w};
    __builtin_nontemporal_store(r, reinterpret_cast<nt_f4*>(a));
}

}  // namespace gsr
