// select_kernels.hip -- the k rows with the smallest row maximum, as flag bytes: the merge's `amax` + `topk(largest=False)` + indexed store.
//
// A row's key is the maximum of its C values mapped to an unsigned integer that orders like the float (NaN largest of all; -0 as +0).  The
// map is monotone, so the key of the maximum is the maximum of the keys: the kernels compare integers and nothing else.  Semantics in
// include/gsr.h (version 121).
//
//   keys      one pass over `values`: every workgroup takes tiles of 256 rows; with C a multiple of 4 the tile is read as consecutive 16-byte
//             pieces (a wave reads 1 KiB per instruction instead of 64 rows 4 C bytes apart) and reduced per row through LDS.  Writes the
//             keys [N] to scratch and the histogram of their highest byte.
//   digit     three more histograms, one per byte, of the rows whose higher bytes equal the bytes chosen so far.  Which byte is chosen
//             follows from the histograms before it; every workgroup works that out for itself at its start (select_resolve: one scan of
//             256 bins per pass), so no launch waits for a choice and no workgroup waits for another one.
//   count     rows equal to the threshold key, per tile of 256 rows
//   scan      one workgroup: exclusive scan of the tile counts in place
//   write     a row is selected when its key is below the threshold key, or equal to it with fewer than `need` equal rows in front of it;
//             drop / keep_flags / meta.
// Histograms: equal digits are combined inside the wave (two rounds of "everybody who holds the first lane's digit", which take a wave of
// equal rows -- the unseen Gaussians, all exactly zero -- in one LDS add), then in the workgroup's LDS histogram, and a workgroup adds only
// its non-zero bins to the global one.  The grid is capped (kSelectGrid workgroups stride over the tiles), so one bin sees at most that many
// global adds per pass.  Integer atomics only: the sums do not depend on their order, a repeat is bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsr.h"

namespace gsr {

int fail_text(int code, const char* text);      // gsr_kernels.hip: sets gsr_last_error()

constexpr int kSelectTile = 256;                // rows per tile: one per thread
constexpr int kSelectGrid = 512;                // workgroups per launch at most (two per CU; they stride over the tiles)
constexpr int kSelectPieces = GSR_SELECT_MAX_COLUMNS / 4;
constexpr uint32_t kSelectNanKey = 0xffffffffu;

// scratch: keys [N] | histograms [4][256] + the NaN counter (+ padding) | tile counts [ntiles]
constexpr int kSelectCounterWords = 4 * 256 + 64;
constexpr int kSelectNanWord = 4 * 256;

__device__ __forceinline__ uint32_t select_key(float v)
{
    // on the bits, so that no floating-point mode (denormals) has a say: NaN = a magnitude above infinity's, zero = a magnitude of 0
    const uint32_t u = __float_as_uint(v), mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u) return kSelectNanKey;
    if (mag == 0u) return 0x80000000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// exclusive prefix of one value per thread over the 256 threads of a workgroup (wave ballots are of no use here: the values are counts)
__device__ __forceinline__ uint32_t select_block_scan(uint32_t v, uint32_t* __restrict__ s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (unsigned int off = 1; off < 256; off <<= 1) {
        const uint32_t add = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t incl = s[threadIdx.x];
    __syncthreads();
    return incl - v;
}

struct SelectChoice {
    uint32_t prefix;      // the bytes chosen by the first `passes` histograms, highest first
    uint32_t need;        // how many rows of the chosen bin are still to be taken (1 .. equal; 0 when k == 0)
    uint32_t below;       // rows in front of the chosen bin
    uint32_t equal;       // rows in the chosen bin
};

// What the first `passes` histograms decide for the k-th smallest key, worked out by all 256 threads of the calling workgroup.
// s: 256 words, pick: 4 words of LDS.  Every index it forms is a thread number below 256.
__device__ SelectChoice select_resolve(const uint32_t* __restrict__ hist, int passes, int64_t k, uint32_t* __restrict__ s,
                                       uint32_t* __restrict__ pick)
{
    SelectChoice c{0u, (uint32_t)k, 0u, 0u};
    if (k <= 0) return c;                         // nothing is selected: threshold key 0, nothing below, nothing equal
    for (int p = 0; p < passes; p++) {
        const uint32_t v = hist[p * 256 + threadIdx.x];
        if (threadIdx.x < 4) pick[threadIdx.x] = 0u;
        const uint32_t excl = select_block_scan(v, s);      // (its barriers order the clear of `pick` before the store below)
        if (v > 0u && excl < c.need && c.need - excl <= v) {
            pick[0] = threadIdx.x;
            pick[1] = excl;
            pick[2] = v;
        }
        __syncthreads();
        c.prefix = (c.prefix << 8) | pick[0];
        c.below += pick[1];
        c.need -= pick[1];
        c.equal = pick[2];
        __syncthreads();
    }
    return c;
}

// One digit per participating lane into the workgroup's LDS histogram.  Called by every lane of the wave (the ballots need them all).
__device__ __forceinline__ void select_hist_add(uint32_t* __restrict__ h, bool valid, uint32_t digit)
{
    const unsigned int lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(valid);
    for (int round = 0; round < 2 && todo; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t d = (uint32_t)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(valid && digit == d);
        if ((int)lane == leader) atomicAdd(&h[d], (uint32_t)__popcll(same));
        if (valid && digit == d) valid = false;
        todo &= ~same;
    }
    if (valid) atomicAdd(&h[digit], 1u);
}

__global__ void k_select_clear(uint32_t* __restrict__ counters)
{
    for (int i = threadIdx.x; i < kSelectCounterWords; i += blockDim.x) counters[i] = 0u;
}

// keys [N] and the histogram of their highest byte.  VEC: C is a multiple of 4 and `values` is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void k_select_keys(const float* __restrict__ values, int64_t N, int32_t C, int64_t ntiles,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ counters)
{
    __shared__ uint32_t h[256];
    __shared__ uint32_t piece_key[VEC ? kSelectTile * kSelectPieces : 1];
    __shared__ uint32_t nan_rows;
    h[threadIdx.x] = 0u;
    if (threadIdx.x == 0) nan_rows = 0u;
    __syncthreads();
    const int32_t P = C >> 2;                    // 16-byte pieces per row (VEC)
    uint32_t my_nan = 0u;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // (the trip count is the same for every thread of the workgroup)
        const int64_t row0 = tile * kSelectTile, i = row0 + threadIdx.x;
        uint32_t key = 0u;
        if (VEC) {
            const int64_t piece0 = row0 * P, pieces = N * (int64_t)P;      // the tile's pieces are consecutive in memory
            const float4* __restrict__ v4 = reinterpret_cast<const float4*>(values);
            for (int32_t j0 = 0; j0 < P; j0 += 4) {              // four loads in flight per lane
                float4 v[4];
#pragma unroll
                for (int32_t u = 0; u < 4; u++) {
                    const int32_t q = (j0 + u) * kSelectTile + (int32_t)threadIdx.x;
                    v[u] = (j0 + u < P && piece0 + q < pieces) ? v4[piece0 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int32_t u = 0; u < 4; u++) {
                    const int32_t q = (j0 + u) * kSelectTile + (int32_t)threadIdx.x;
                    if (j0 + u < P && piece0 + q < pieces)
                        piece_key[q] = umax32(umax32(select_key(v[u].x), select_key(v[u].y)), umax32(select_key(v[u].z), select_key(v[u].w)));
                }
            }
            __syncthreads();
            if (i < N)
                for (int32_t j = 0; j < P; j++) key = umax32(key, piece_key[(int32_t)threadIdx.x * P + j]);
            __syncthreads();
        } else if (i < N) {
            const float* __restrict__ row = values + i * (int64_t)C;
            for (int32_t j = 0; j < C; j++) key = umax32(key, select_key(row[j]));
        }
        if (i < N) {
            keys[i] = key;
            my_nan += key == kSelectNanKey ? 1u : 0u;
        }
        select_hist_add(h, i < N, key >> 24);
    }
    if (my_nan) atomicAdd(&nan_rows, my_nan);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&counters[threadIdx.x], h[threadIdx.x]);
    if (threadIdx.x == 0 && nan_rows) atomicAdd(&counters[kSelectNanWord], nan_rows);
}

// histogram `pass` (1, 2, 3): the next byte of the rows whose higher bytes are the ones chosen so far
__global__ __launch_bounds__(256) void k_select_digit(const uint32_t* __restrict__ keys, int64_t N, int64_t ntiles, int64_t k, int pass,
                                                      uint32_t* __restrict__ counters)
{
    __shared__ uint32_t h[256];
    __shared__ uint32_t s[256];
    __shared__ uint32_t pick[4];
    const SelectChoice c = select_resolve(counters, pass, k, s, pick);
    if (k <= 0) return;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int high = 32 - 8 * pass, shift = 24 - 8 * pass;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kSelectTile + threadIdx.x;
        const uint32_t key = i < N ? keys[i] : 0u;
        select_hist_add(h, i < N && (key >> high) == c.prefix, (key >> shift) & 255u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&counters[pass * 256 + threadIdx.x], h[threadIdx.x]);
}

// the number of rows of the tile for which `flag` holds in front of the calling thread, *total the tile's number
__device__ __forceinline__ uint32_t select_tile_rank(bool flag, uint32_t* __restrict__ wave_total, uint32_t* total)
{
    const unsigned long long b = __ballot(flag);
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1ull)), sum = 0u;
    for (unsigned int w = 0; w < 4; w++) {
        if (w < wave) before += wave_total[w];
        sum += wave_total[w];
    }
    *total = sum;
    __syncthreads();
    return before;
}

__global__ __launch_bounds__(256) void k_select_count(const uint32_t* __restrict__ keys, int64_t N, int64_t ntiles, int64_t k,
                                                      const uint32_t* __restrict__ counters, uint32_t* __restrict__ tile_count)
{
    __shared__ uint32_t s[256];
    __shared__ uint32_t pick[4];
    __shared__ uint32_t wave_total[4];
    const SelectChoice c = select_resolve(counters, 4, k, s, pick);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kSelectTile + threadIdx.x;
        uint32_t total;
        select_tile_rank(k > 0 && i < N && keys[i] == c.prefix, wave_total, &total);
        if (threadIdx.x == 0) tile_count[tile] = total;
    }
}

__global__ __launch_bounds__(256) void k_select_scan_tiles(uint32_t* __restrict__ tile_count, int64_t ntiles)
{
    __shared__ uint32_t s[256];
    uint32_t running = 0u;
    for (int64_t lo = 0; lo < ntiles; lo += 256) {
        const int64_t t = lo + threadIdx.x;
        const uint32_t v = t < ntiles ? tile_count[t] : 0u;
        const uint32_t excl = select_block_scan(v, s);
        if (t < ntiles) tile_count[t] = running + excl;
        s[threadIdx.x] = excl + v;
        __syncthreads();
        running += s[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_select_write(const uint32_t* __restrict__ keys, int64_t N, int64_t ntiles, int64_t k,
                                                      const uint32_t* __restrict__ counters, const uint32_t* __restrict__ tile_offset,
                                                      uint8_t* __restrict__ drop, uint8_t* __restrict__ keep_flags, int64_t* __restrict__ meta)
{
    __shared__ uint32_t s[256];
    __shared__ uint32_t pick[4];
    __shared__ uint32_t wave_total[4];
    const SelectChoice c = select_resolve(counters, 4, k, s, pick);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kSelectTile + threadIdx.x;
        const uint32_t key = i < N ? keys[i] : 0u;
        const bool tie = k > 0 && i < N && key == c.prefix;
        uint32_t total;
        const uint32_t rank = tile_offset[tile] + select_tile_rank(tie, wave_total, &total);
        if (i < N) {                                  // the only addresses formed here are row numbers below N
            const bool taken = k > 0 && (key < c.prefix || (tie && rank < c.need));
            if (drop) drop[i] = taken ? 1 : 0;
            if (keep_flags) keep_flags[i] = taken ? 0 : GSR_RESIZE_KEEP;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        meta[0] = k;
        meta[1] = (int64_t)c.below;
        meta[2] = (int64_t)c.equal;
        meta[3] = (int64_t)c.prefix;
        meta[4] = (int64_t)counters[kSelectNanWord];
        meta[5] = 0;
        meta[6] = 0;
        meta[7] = 0;
    }
}

__global__ void k_select_meta_empty(int64_t* __restrict__ meta)
{
    if (threadIdx.x < GSR_SELECT_META_WORDS) meta[threadIdx.x] = 0;
}

static inline int64_t select_tiles(int64_t N) { return (N + kSelectTile - 1) / kSelectTile; }
static inline size_t select_keys_bytes(int64_t N) { return ((size_t)N * sizeof(uint32_t) + 255) & ~(size_t)255; }

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_select_scratch_bytes(int64_t N)
{
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) N = ((int64_t)1 << 31) - 1;      // (larger inputs are refused by the call itself)
    return select_keys_bytes(N) + (size_t)kSelectCounterWords * sizeof(uint32_t) + (((size_t)select_tiles(N) * sizeof(uint32_t) + 255) & ~(size_t)255);
}

int gsr_select_smallest(const float* values, int64_t N, int32_t C, int64_t k, uint8_t* drop, uint8_t* keep_flags, int64_t* meta, void* scratch,
                        size_t scratch_bytes, void* stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31)) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: N must be in [0, 2^31) (a plan's row numbers are int32)");
    if (C < 1 || C > GSR_SELECT_MAX_COLUMNS) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: C must be in [1, GSR_SELECT_MAX_COLUMNS (64)]");
    if (k < 0 || k > N) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: k must be in [0, N]");
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: meta is NULL or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        hipLaunchKernelGGL(k_select_meta_empty, dim3(1), dim3(64), 0, st, meta);
        return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
    }
    if (!drop && !keep_flags) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: drop and keep_flags are both NULL");
    if (!values || ((uintptr_t)values & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: values is NULL or not 4-byte aligned");
    if (!scratch || ((uintptr_t)scratch & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_select_smallest: scratch is NULL or not 4-byte aligned");
    if (scratch_bytes < gsr_select_scratch_bytes(N))
        return fail_text(GSR_ERR_ARG, "gsr_select_smallest: scratch is shorter than gsr_select_scratch_bytes(N)");
    const int64_t ntiles = select_tiles(N);
    const unsigned grid = (unsigned)(ntiles < kSelectGrid ? ntiles : kSelectGrid);
    uint32_t* keys = static_cast<uint32_t*>(scratch);
    uint32_t* counters = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + select_keys_bytes(N));
    uint32_t* tiles = counters + kSelectCounterWords;
    hipLaunchKernelGGL(k_select_clear, dim3(1), dim3(256), 0, st, counters);
    if ((C & 3) == 0 && ((uintptr_t)values & 15) == 0)
        hipLaunchKernelGGL(k_select_keys<true>, dim3(grid), dim3(256), 0, st, values, N, C, ntiles, keys, counters);
    else
        hipLaunchKernelGGL(k_select_keys<false>, dim3(grid), dim3(256), 0, st, values, N, C, ntiles, keys, counters);
    for (int pass = 1; pass < 4; pass++)
        hipLaunchKernelGGL(k_select_digit, dim3(grid), dim3(256), 0, st, keys, N, ntiles, k, pass, counters);
    hipLaunchKernelGGL(k_select_count, dim3(grid), dim3(256), 0, st, keys, N, ntiles, k, counters, tiles);
    hipLaunchKernelGGL(k_select_scan_tiles, dim3(1), dim3(256), 0, st, tiles, ntiles);
    hipLaunchKernelGGL(k_select_write, dim3(grid), dim3(256), 0, st, keys, N, ntiles, k, counters, tiles, drop, keep_flags, meta);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
