// voxel_kernels.hip -- the single-image model's point cloud on the device: depth map -> points -> voxel-grid means.
//
// The reference builds it on the host for every frame of stage A and every leaf (/root/reference/trainer/trainer.py:646-671):
// kornia.depth_to_3d on the device, a copy of H*W points to the host, open3d voxel_down_sample(voxel_size=0.01), a copy back, then
// create_from_pcd (/root/reference/scene/gaussian_model_ht.py:197-233), whose distCUDA2 is knn_kernels.hip.  These are the two steps in
// front of it; their semantics are pinned in include/gsr.h (restatements of the public kornia / Open3D definitions: neither
// library is available to the tests).
//
//   gsr_depth_to_points    one lane per pixel: two float32 roundings and a product per coordinate, nothing that contracts to an FMA.
//   gsr_voxel_down_sample  1. bounds   min / max over the finite points (two-stage, no atomics), count of the dropped ones, the
//                                      overflow status from the largest index of each axis (floor is monotone: the maximum decides);
//                          2. keys     ix<<42 | iy<<21 | iz in float64; all ones for a non-finite point (sorts last);
//                          3. sort     stable, 63 bits as two 32-bit sorts of the library's own (gsr_sort_pairs_u32): low word, gather
//                                      of the high word, high word.  Stable => inside a voxel the points stay in input order;
//                          4. heads    segment heads flagged on the sorted keys, scanned in three launches (count per tile, one
//                                      workgroup over the tile counts, write) -> voxel number, segment starts, M;
//                          5. means    float64 sums in an order that depends on the segment's LENGTH alone: up to kVoxLane points one lane
//                                      adds them in input order; up to kVoxWave a wave (lane l adds l, l+64, ..., then a shuffle tree);
//                                      longer ones a workgroup of four waves, the same per wave plus ((w0+w1)+(w2+w3)).  No float
//                                      atomics anywhere; the two integer atomics only build the work lists of the long segments, whose
//                                      order changes which wave serves a segment and nothing of what it computes.
// No workgroup of this file waits for another one inside a launch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "../../include/gsr.h"

namespace gsr {

constexpr int kVoxTile = 2048;          // sorted positions per workgroup of the head scan (256 threads x 8)
constexpr int kVoxLane = 16;            // longest segment one lane sums
constexpr int kVoxWave = 2048;          // longest segment one wave sums
constexpr int kVoxPartials = 256;       // workgroups of the bounds pass
constexpr uint64_t kVoxNoKey = ~0ull;   // key of a point that belongs to no voxel
constexpr int kVoxLongGrid = 1024;      // workgroups of the two long-segment launches (they stride over their lists)

// what the chain keeps between its launches (head of the scratch)
struct VoxState {
    double origin[3];
    float mn[3], mx[3];
    unsigned long long nvalid;
    unsigned int status;
    unsigned int n_wave, n_block;       // lengths of the two long-segment lists
    unsigned int M;
};

__global__ __launch_bounds__(256) void k_depth_to_points(const float* __restrict__ depth, const float* __restrict__ image, int H, int W,
                                                         float fx, float fy, float cx, float cy, float* __restrict__ points,
                                                         float* __restrict__ colors)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int v = (int)(i / W), u = (int)(i - (int64_t)v * W);
    const float d = depth[i];
    // ((u - cx) / fx) * d: a subtraction, a division, a product -- three roundings, no multiply-add for the compiler to contract
    const float xn = ((float)u - cx) / fx, yn = ((float)v - cy) / fy;
    points[3 * i] = xn * d;
    points[3 * i + 1] = yn * d;
    points[3 * i + 2] = d;
    if (colors) {
        colors[3 * i] = image[i];
        colors[3 * i + 1] = image[HW + i];
        colors[3 * i + 2] = image[2 * HW + i];
    }
}

__device__ __forceinline__ bool vox_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// partial: [block][8] = min xyz, max xyz, dropped (as uint bits), unused
__global__ __launch_bounds__(256) void k_vox_bounds_partial(const float* __restrict__ p, int64_t N, float* __restrict__ partial)
{
    __shared__ float s[6][256];
    __shared__ unsigned int sd[256];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned int dropped = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (!vox_finite(x, y, z)) { dropped++; continue; }
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    for (int k = 0; k < 3; k++) { s[k][threadIdx.x] = mn[k]; s[3 + k][threadIdx.x] = mx[k]; }
    sd[threadIdx.x] = dropped;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            for (int k = 0; k < 3; k++) {
                s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + off]);
                s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + off]);
            }
            sd[threadIdx.x] += sd[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[blockIdx.x * 8 + threadIdx.x] = s[threadIdx.x][0];
    if (threadIdx.x == 6) partial[blockIdx.x * 8 + 6] = __uint_as_float(sd[0]);
}

// one wave: the bounds, the origin, the status and the call's counters
__global__ void k_vox_bounds_finish(const float* __restrict__ partial, int nb, int64_t N, double voxel_size, VoxState* __restrict__ st,
                                    int64_t* __restrict__ meta)
{
    if (threadIdx.x != 0) return;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned long long dropped = 0;
    for (int b = 0; b < nb; b++) {
        for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], partial[b * 8 + k]); mx[k] = fmaxf(mx[k], partial[b * 8 + 3 + k]); }
        dropped += __float_as_uint(partial[b * 8 + 6]);
    }
    const unsigned long long nvalid = (unsigned long long)N - dropped;
    unsigned int status = 0;
    for (int k = 0; k < 3; k++) {
        const double origin = nvalid ? (double)mn[k] - 0.5 * voxel_size : 0.0;
        st->origin[k] = origin; st->mn[k] = mn[k]; st->mx[k] = mx[k];
        if (nvalid) {
            const double top = floor(((double)mx[k] - origin) / voxel_size);
            if (!(top < 2097152.0)) status = 1;      // an index >= 2^21 (or an extent that overflowed to infinity)
        }
    }
    st->nvalid = nvalid; st->status = status; st->n_wave = 0; st->n_block = 0; st->M = 0;
    meta[1] = (int64_t)dropped; meta[2] = (int64_t)status; meta[3] = 0;
    if (status || !nvalid) meta[0] = 0;              // (otherwise the head scan writes M)
}

__global__ __launch_bounds__(256) void k_vox_keys(const float* __restrict__ p, int64_t N, double voxel_size, const VoxState* __restrict__ st,
                                                  uint64_t* __restrict__ key64, uint32_t* __restrict__ klo, uint32_t* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float c[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    uint64_t key = kVoxNoKey;
    if (vox_finite(c[0], c[1], c[2])) {
        key = 0;
        for (int k = 0; k < 3; k++) {
            double f = floor(((double)c[k] - st->origin[k]) / voxel_size);
            f = f < 0.0 ? 0.0 : (f > 2097151.0 ? 2097151.0 : f);     // (only reached with status 1, whose rows nobody relies on)
            key = (key << 21) | (uint64_t)f;
        }
    }
    key64[i] = key;
    klo[i] = (uint32_t)key;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_vox_gather_hi(const uint64_t* __restrict__ key64, const uint32_t* __restrict__ order, int64_t N,
                                                       uint32_t* __restrict__ khi)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) khi[j] = (uint32_t)(key64[order[j]] >> 32);
}

__global__ __launch_bounds__(256) void k_vox_gather_key(const uint64_t* __restrict__ key64, const uint32_t* __restrict__ order, int64_t N,
                                                        uint64_t* __restrict__ skey)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) skey[j] = key64[order[j]];
}

__device__ __forceinline__ bool vox_is_head(const uint64_t* __restrict__ skey, int64_t j, int64_t nvalid)
{
    return j < nvalid && (j == 0 || skey[j] != skey[j - 1]);
}

// sum of one value per thread over the 256 threads of a workgroup, and the exclusive prefix of the caller's own value
__device__ __forceinline__ unsigned int vox_block_scan(unsigned int v, unsigned int* __restrict__ s, unsigned int* total)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned int add = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned int incl = s[threadIdx.x];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_vox_head_count(const uint64_t* __restrict__ skey, int64_t N, const VoxState* __restrict__ st,
                                                        unsigned int* __restrict__ tile_count)
{
    __shared__ unsigned int s[256];
    const int64_t nvalid = (int64_t)st->nvalid;
    const int64_t base = (int64_t)blockIdx.x * kVoxTile + (int64_t)threadIdx.x * 8;
    unsigned int c = 0;
    for (int q = 0; q < 8; q++)
        if (base + q < N && vox_is_head(skey, base + q, nvalid)) c++;
    unsigned int total;
    vox_block_scan(c, s, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile counts in place, M
__global__ __launch_bounds__(256) void k_vox_scan_tiles(unsigned int* __restrict__ tile_count, int64_t ntiles, VoxState* __restrict__ st,
                                                        uint32_t* __restrict__ seg_start, int64_t* __restrict__ meta)
{
    __shared__ unsigned int s[256];
    unsigned int running = 0;
    for (int64_t lo = 0; lo < ntiles; lo += 256) {
        const int64_t t = lo + threadIdx.x;
        const unsigned int v = t < ntiles ? tile_count[t] : 0u;
        unsigned int total;
        const unsigned int excl = vox_block_scan(v, s, &total);
        if (t < ntiles) tile_count[t] = running + excl;
        running += total;
    }
    if (threadIdx.x == 0) {
        const unsigned int M = st->status ? 0u : running;
        st->M = M;
        seg_start[running] = (uint32_t)st->nvalid;     // the end of the last segment
        meta[0] = (int64_t)M;
    }
}

__global__ __launch_bounds__(256) void k_vox_head_write(const uint64_t* __restrict__ skey, int64_t N, const VoxState* __restrict__ st,
                                                        const unsigned int* __restrict__ tile_offset, uint32_t* __restrict__ seg_start)
{
    __shared__ unsigned int s[256];
    const int64_t nvalid = (int64_t)st->nvalid;
    const int64_t base = (int64_t)blockIdx.x * kVoxTile + (int64_t)threadIdx.x * 8;
    bool head[8];
    unsigned int c = 0;
    for (int q = 0; q < 8; q++) {
        head[q] = base + q < N && vox_is_head(skey, base + q, nvalid);
        c += head[q] ? 1u : 0u;
    }
    unsigned int total;
    unsigned int id = tile_offset[blockIdx.x] + vox_block_scan(c, s, &total);
    for (int q = 0; q < 8; q++)
        if (head[q]) seg_start[id++] = (uint32_t)(base + q);
}

struct VoxSum { double p[3], c[3]; };

__device__ __forceinline__ void vox_add(VoxSum& a, const float* __restrict__ points, const float* __restrict__ colors, uint32_t i)
{
    a.p[0] += (double)points[3 * (size_t)i]; a.p[1] += (double)points[3 * (size_t)i + 1]; a.p[2] += (double)points[3 * (size_t)i + 2];
    if (colors) { a.c[0] += (double)colors[3 * (size_t)i]; a.c[1] += (double)colors[3 * (size_t)i + 1]; a.c[2] += (double)colors[3 * (size_t)i + 2]; }
}

__device__ __forceinline__ void vox_store(const VoxSum& a, uint32_t len, uint32_t m, bool with_colors, float* __restrict__ out_points,
                                          float* __restrict__ out_colors, int32_t* __restrict__ out_counts)
{
    const double n = (double)len;
    for (int k = 0; k < 3; k++) out_points[3 * (size_t)m + k] = (float)(a.p[k] / n);
    if (with_colors) for (int k = 0; k < 3; k++) out_colors[3 * (size_t)m + k] = (float)(a.c[k] / n);
    if (out_counts) out_counts[m] = (int32_t)len;
}

// a wave's sum of the segment [lo, lo + len): lane l adds positions l, l + 64, ... in order, then the lanes fold 32, 16, ..., 1 apart
__device__ __forceinline__ VoxSum vox_wave_sum(const float* __restrict__ points, const float* __restrict__ colors,
                                               const uint32_t* __restrict__ order, uint32_t lo, uint32_t len, uint32_t first, uint32_t stride)
{
    VoxSum a = {};
    for (uint32_t q = first; q < len; q += stride) vox_add(a, points, colors, order[lo + q]);
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 3; k++) {
            a.p[k] += __shfl_down(a.p[k], off, 64);
            if (colors) a.c[k] += __shfl_down(a.c[k], off, 64);
        }
    return a;      // complete in lane 0
}

// a lane per voxel: short segments are summed here, long ones are put on the wave's or the workgroup's list
__global__ __launch_bounds__(256) void k_vox_means(const float* __restrict__ points, const float* __restrict__ colors,
                                                   const uint32_t* __restrict__ order, const uint32_t* __restrict__ seg_start, int64_t N,
                                                   VoxState* __restrict__ st, uint32_t* __restrict__ list_wave, uint32_t* __restrict__ list_block,
                                                   float* __restrict__ out_points, float* __restrict__ out_colors, int32_t* __restrict__ out_counts)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= (int64_t)st->M) return;
    const uint32_t lo = seg_start[m], len = seg_start[m + 1] - lo;
    if (len > (uint32_t)kVoxWave) { list_block[atomicAdd(&st->n_block, 1u)] = (uint32_t)m; return; }
    if (len > (uint32_t)kVoxLane) { list_wave[atomicAdd(&st->n_wave, 1u)] = (uint32_t)m; return; }
    VoxSum a = {};
    for (uint32_t q = 0; q < len; q++) vox_add(a, points, colors, order[lo + q]);
    vox_store(a, len, (uint32_t)m, colors != nullptr, out_points, out_colors, out_counts);
}

__global__ __launch_bounds__(256) void k_vox_means_wave(const float* __restrict__ points, const float* __restrict__ colors,
                                                        const uint32_t* __restrict__ order, const uint32_t* __restrict__ seg_start,
                                                        const VoxState* __restrict__ st, const uint32_t* __restrict__ list_wave,
                                                        float* __restrict__ out_points, float* __restrict__ out_colors, int32_t* __restrict__ out_counts)
{
    const uint32_t lane = threadIdx.x & 63, n = st->n_wave;
    for (uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n; s += gridDim.x * 4) {
        const uint32_t m = list_wave[s], lo = seg_start[m], len = seg_start[m + 1] - lo;
        const VoxSum a = vox_wave_sum(points, colors, order, lo, len, lane, 64);
        if (lane == 0) vox_store(a, len, m, colors != nullptr, out_points, out_colors, out_counts);
    }
}

__global__ __launch_bounds__(256) void k_vox_means_block(const float* __restrict__ points, const float* __restrict__ colors,
                                                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ seg_start,
                                                         const VoxState* __restrict__ st, const uint32_t* __restrict__ list_block,
                                                         float* __restrict__ out_points, float* __restrict__ out_colors, int32_t* __restrict__ out_counts)
{
    __shared__ VoxSum part[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = st->n_block;
    for (uint32_t s = blockIdx.x; s < n; s += gridDim.x) {
        const uint32_t m = list_block[s], lo = seg_start[m], len = seg_start[m + 1] - lo;
        // thread t adds positions t, t + 256, ...; each wave folds its 64 lanes, thread 0 adds the four waves as (w0 + w1) + (w2 + w3)
        const VoxSum a = vox_wave_sum(points, colors, order, lo, len, threadIdx.x, 256);
        if (lane == 0) part[wave] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            VoxSum t = {};
            for (int k = 0; k < 3; k++) {
                t.p[k] = (part[0].p[k] + part[1].p[k]) + (part[2].p[k] + part[3].p[k]);
                t.c[k] = (part[0].c[k] + part[1].c[k]) + (part[2].c[k] + part[3].c[k]);
            }
            vox_store(t, len, m, colors != nullptr, out_points, out_colors, out_counts);
        }
        __syncthreads();
    }
}

__global__ void k_vox_meta_zero(int64_t* __restrict__ meta)
{
    if (threadIdx.x < 4) meta[threadIdx.x] = 0;
}

static inline size_t v256(size_t x) { return (x + 255) & ~(size_t)255; }

struct VoxLayout {
    size_t state, partial, key64, skey, k0, k1, v0, v1, seg_start, tiles, list_wave, list_block, sort, sort_bytes, bytes;
};

static VoxLayout vox_layout(int64_t N)
{
    VoxLayout L{};
    const size_t n = (size_t)N;
    size_t o = 0;
    L.state = o; o += v256(sizeof(VoxState));
    L.partial = o; o += v256((size_t)kVoxPartials * 8 * 4);
    L.key64 = o; o += v256(n * 8);
    L.skey = o; o += v256(n * 8);
    L.k0 = o; o += v256(n * 4);
    L.k1 = o; o += v256(n * 4);
    L.v0 = o; o += v256(n * 4);
    L.v1 = o; o += v256(n * 4);
    L.seg_start = o; o += v256((n + 1) * 4);
    L.tiles = o; o += v256(((n + kVoxTile - 1) / kVoxTile + 1) * 4);
    L.list_wave = o; o += v256((n / (kVoxLane + 1) + 1) * 4);
    L.list_block = o; o += v256((n / (kVoxWave + 1) + 1) * 4);
    L.sort = o; L.sort_bytes = gsr_sort_scratch_bytes((uint32_t)n); o += v256(L.sort_bytes);
    L.bytes = o;
    return L;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_depth_to_points(const float* depth, const float* image, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float* points,
                        float* colors, void* stream)
{
    if (!depth || !points || H <= 0 || W <= 0 || fx == 0.f || fy == 0.f || (image != nullptr) != (colors != nullptr)) return GSR_ERR_ARG;
    const int64_t HW = (int64_t)H * W;
    if (HW >= ((int64_t)1 << 31)) return GSR_ERR_ARG;
    hipLaunchKernelGGL(k_depth_to_points, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, image, H, W, fx, fy,
                       cx, cy, points, colors);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

size_t gsr_voxel_scratch_bytes(int64_t N)
{
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) N = ((int64_t)1 << 31) - 1;      // (larger clouds are refused by the call itself)
    return vox_layout(N).bytes;
}

int gsr_voxel_down_sample(const float* points, const float* colors, int64_t N, double voxel_size, float* out_points, float* out_colors,
                          int32_t* out_counts, int64_t* meta, void* scratch, size_t scratch_bytes, void* stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31) || !meta || ((uintptr_t)meta & 7) != 0) return GSR_ERR_ARG;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) return GSR_ERR_ARG;
    if ((colors != nullptr) != (out_colors != nullptr)) return GSR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        hipLaunchKernelGGL(k_vox_meta_zero, dim3(1), dim3(64), 0, st, meta);
        return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
    }
    if (!points || !out_points || !scratch || ((uintptr_t)scratch & 7) != 0 || scratch_bytes < gsr_voxel_scratch_bytes(N)) return GSR_ERR_ARG;
    const VoxLayout L = vox_layout(N);
    uint8_t* s = static_cast<uint8_t*>(scratch);
    VoxState* state = reinterpret_cast<VoxState*>(s + L.state);
    float* partial = reinterpret_cast<float*>(s + L.partial);
    uint64_t* key64 = reinterpret_cast<uint64_t*>(s + L.key64);
    uint64_t* skey = reinterpret_cast<uint64_t*>(s + L.skey);
    uint32_t* k0 = reinterpret_cast<uint32_t*>(s + L.k0);
    uint32_t* k1 = reinterpret_cast<uint32_t*>(s + L.k1);
    uint32_t* v0 = reinterpret_cast<uint32_t*>(s + L.v0);
    uint32_t* v1 = reinterpret_cast<uint32_t*>(s + L.v1);
    uint32_t* seg_start = reinterpret_cast<uint32_t*>(s + L.seg_start);
    unsigned int* tiles = reinterpret_cast<unsigned int*>(s + L.tiles);
    uint32_t* list_wave = reinterpret_cast<uint32_t*>(s + L.list_wave);
    uint32_t* list_block = reinterpret_cast<uint32_t*>(s + L.list_block);
    void* sort_scratch = s + L.sort;

    const unsigned grid = (unsigned)((N + 255) / 256);
    const int nb = (int)(grid < (unsigned)kVoxPartials ? grid : (unsigned)kVoxPartials);
    const int64_t ntiles = (N + kVoxTile - 1) / kVoxTile;
    hipLaunchKernelGGL(k_vox_bounds_partial, dim3(nb), dim3(256), 0, st, points, N, partial);
    hipLaunchKernelGGL(k_vox_bounds_finish, dim3(1), dim3(64), 0, st, partial, nb, N, voxel_size, state, meta);
    hipLaunchKernelGGL(k_vox_keys, dim3(grid), dim3(256), 0, st, points, N, voxel_size, state, key64, k0, v0);
    int in_alt = 0;
    if (gsr_sort_pairs_u32(k0, v0, k1, v1, (uint32_t)N, 0, 32, sort_scratch, L.sort_bytes, &in_alt, stream) != GSR_OK) return GSR_ERR_HIP;
    uint32_t *ka = in_alt ? k1 : k0, *va = in_alt ? v1 : v0, *kb = in_alt ? k0 : k1, *vb = in_alt ? v0 : v1;
    hipLaunchKernelGGL(k_vox_gather_hi, dim3(grid), dim3(256), 0, st, key64, va, N, ka);
    if (gsr_sort_pairs_u32(ka, va, kb, vb, (uint32_t)N, 0, 32, sort_scratch, L.sort_bytes, &in_alt, stream) != GSR_OK) return GSR_ERR_HIP;
    const uint32_t* order = in_alt ? vb : va;
    hipLaunchKernelGGL(k_vox_gather_key, dim3(grid), dim3(256), 0, st, key64, order, N, skey);
    hipLaunchKernelGGL(k_vox_head_count, dim3((unsigned)ntiles), dim3(256), 0, st, skey, N, state, tiles);
    hipLaunchKernelGGL(k_vox_scan_tiles, dim3(1), dim3(256), 0, st, tiles, ntiles, state, seg_start, meta);
    hipLaunchKernelGGL(k_vox_head_write, dim3((unsigned)ntiles), dim3(256), 0, st, skey, N, state, tiles, seg_start);
    hipLaunchKernelGGL(k_vox_means, dim3(grid), dim3(256), 0, st, points, colors, order, seg_start, N, state, list_wave, list_block,
                       out_points, out_colors, out_counts);
    hipLaunchKernelGGL(k_vox_means_wave, dim3(kVoxLongGrid), dim3(256), 0, st, points, colors, order, seg_start, state, list_wave,
                       out_points, out_colors, out_counts);
    hipLaunchKernelGGL(k_vox_means_block, dim3(kVoxLongGrid), dim3(256), 0, st, points, colors, order, seg_start, state, list_block,
                       out_points, out_colors, out_counts);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
