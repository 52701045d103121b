// resize_kernels.hip -- resizing the model on the device: prune, clone and split as one layout decision and one row move.
//
// Densification and pruning (densify.py, train_step.GaussianParams) replace the six parameter tensors and their Adam moments by tensors of
// another length.  What the new tensors hold is decided by one flag byte per row; the kernels of this file turn the flag bytes into the
// source-row lists of the new layout (the plan) and then move the rows.  They compute no float: every byte of the result is a copy of a byte
// the caller supplied, or zero.  Semantics in include/gsr.h (version 120).
//
//   gsr_resize_plan    count     one workgroup per tile of kResizeTile rows: how many rows of the tile enter each of the four lists;
//                      scan      four workgroups, one per list: exclusive scan of its tile counts in place, the list's length to meta;
//                      write     the tile again: every row's position inside its lists = the tile's offset + its rank in the tile.
//                      (the count -> scan -> write shape of voxel_kernels.hip's segment heads)
//   gsr_resize_apply   one launch; blockIdx.y picks the tensor, the x dimension strides over the tensor's destination in 4-byte words, so a
//                      wave stores 256 consecutive bytes.  Every row number read from the plan is compared against N before it is used as
//                      an address: a row that fails is written as zeros and raises meta[4].
//   gsr_merge_apply    (version 121) the same launch over two models: the A lists of two plans name the rows of the appended result.
//   gsr_resize_plan_batched / gsr_resize_apply_batched   (version 122) the plan and the apply over the B models of a batched store: count,
//                      scan and write per 128-row block (a block belongs to one model), the scan on a (list, model) grid; the apply strides
//                      over the blocks of the new store and writes its padding rows too.  The number of launches does not depend on B.
// No workgroup of this file waits for another one inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gsr.h"

namespace gsr {

int fail_text(int code, const char* text);      // gsr_kernels.hip: sets gsr_last_error()

constexpr int kResizeTile = 256;                // rows per workgroup of the plan: one per thread
constexpr int kResizeApplyGridX = 2048;         // workgroups per tensor of the apply launch at most (they stride)

struct ResizeTable {
    GsrResizeTensor t[GSR_RESIZE_MAX_TENSORS];
};

// list membership of one flag byte, one 16-bit field per list (a tile holds at most 256 of each): A | B << 16 | C << 32 | S << 48
__device__ __forceinline__ unsigned long long resize_fields(uint8_t f)
{
    const unsigned long long a = (f & GSR_RESIZE_KEEP) ? 1ull : 0ull;
    const unsigned long long b = (f & GSR_RESIZE_CLONE) ? 1ull : 0ull;
    const unsigned long long s = (f & GSR_RESIZE_SPLIT) ? 1ull : 0ull;
    const unsigned long long c = ((f & GSR_RESIZE_SPLIT) && (f & GSR_RESIZE_CHILD)) ? 1ull : 0ull;
    return a | (b << 16) | (c << 32) | (s << 48);
}

// inclusive scan of one value per thread over the 256 threads of a workgroup; returns the caller's exclusive prefix, *total the sum
template <typename T>
__device__ __forceinline__ T resize_block_scan(T v, T* __restrict__ s, T* total)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (unsigned int off = 1; off < 256; off <<= 1) {
        const T add = threadIdx.x >= off ? s[threadIdx.x - off] : (T)0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const T incl = s[threadIdx.x];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// tile_count: [4][ntiles]
__global__ __launch_bounds__(256) void k_resize_count(const uint8_t* __restrict__ flags, int64_t N, int64_t ntiles,
                                                      unsigned int* __restrict__ tile_count)
{
    __shared__ unsigned long long s[256];
    const int64_t i = (int64_t)blockIdx.x * kResizeTile + threadIdx.x;
    const unsigned long long v = i < N ? resize_fields(flags[i]) : 0ull;
    unsigned long long total;
    resize_block_scan(v, s, &total);
    if (threadIdx.x < 4) tile_count[(int64_t)threadIdx.x * ntiles + blockIdx.x] = (unsigned int)((total >> (16 * threadIdx.x)) & 0xffffull);
}

// workgroup b: exclusive scan of list b's tile counts in place, its length to meta[b]; workgroup 0 also clears the status words
__global__ __launch_bounds__(256) void k_resize_scan_tiles(unsigned int* __restrict__ tile_count, int64_t ntiles, int64_t* __restrict__ meta)
{
    __shared__ unsigned int s[256];
    unsigned int* tc = tile_count + (int64_t)blockIdx.x * ntiles;
    unsigned int running = 0;
    for (int64_t lo = 0; lo < ntiles; lo += 256) {
        const int64_t t = lo + threadIdx.x;
        const unsigned int v = t < ntiles ? tc[t] : 0u;
        unsigned int total;
        const unsigned int excl = resize_block_scan(v, s, &total);
        if (t < ntiles) tc[t] = running + excl;
        running += total;
    }
    if (threadIdx.x == 0) meta[blockIdx.x] = (int64_t)running;
    if (blockIdx.x == 0 && threadIdx.x >= 4 && threadIdx.x < GSR_RESIZE_META_WORDS) meta[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void k_resize_write(const uint8_t* __restrict__ flags, int64_t N, int64_t ntiles,
                                                      const unsigned int* __restrict__ tile_offset, int32_t* __restrict__ plan, int64_t stride)
{
    __shared__ unsigned long long s[256];
    const int64_t i = (int64_t)blockIdx.x * kResizeTile + threadIdx.x;
    const unsigned long long v = i < N ? resize_fields(flags[i]) : 0ull;
    unsigned long long total;
    const unsigned long long excl = resize_block_scan(v, s, &total);
    if (i >= N) return;
    // positions are below N (a list holds each row at most once), so every store stays inside its N-entry segment
    const unsigned int pa = tile_offset[blockIdx.x] + (unsigned int)(excl & 0xffffull);
    const unsigned int pb = tile_offset[ntiles + blockIdx.x] + (unsigned int)((excl >> 16) & 0xffffull);
    const unsigned int pc = tile_offset[2 * ntiles + blockIdx.x] + (unsigned int)((excl >> 32) & 0xffffull);
    const unsigned int ps = tile_offset[3 * ntiles + blockIdx.x] + (unsigned int)((excl >> 48) & 0xffffull);
    // (the comparisons with N hold whenever the flags are the bytes the count pass saw; they keep a caller's race inside the buffer)
    const unsigned int n = (unsigned int)N;
    if ((v & 0xffffull) && pa < n) plan[GSR_RESIZE_PLAN_ROWS_A * stride + pa] = (int32_t)i;
    if (((v >> 16) & 0xffffull) && pb < n) plan[GSR_RESIZE_PLAN_ROWS_B * stride + pb] = (int32_t)i;
    if (((v >> 32) & 0xffffull) && pc < n) {
        plan[GSR_RESIZE_PLAN_ROWS_C * stride + pc] = (int32_t)i;
        plan[GSR_RESIZE_PLAN_RANK_C * stride + pc] = (int32_t)ps;
    }
    if (((v >> 48) & 0xffffull) && ps < n) plan[GSR_RESIZE_PLAN_SPLIT_ROWS * stride + ps] = (int32_t)i;
}

__global__ void k_resize_meta_zero(int64_t* __restrict__ meta)
{
    if (threadIdx.x < GSR_RESIZE_META_WORDS) meta[threadIdx.x] = 0;
}

// grid (x, count): tensor blockIdx.y, destination words e = row * words + w
__global__ __launch_bounds__(256) void k_resize_apply(const int32_t* __restrict__ plan, int64_t stride, int64_t N, int64_t nA, int64_t nB,
                                                      int64_t nC, int64_t nSplit, ResizeTable table, int64_t* __restrict__ meta)
{
    const GsrResizeTensor T = table.t[blockIdx.y];
    if (!T.src || !T.dst || T.row_bytes <= 0) return;
    const uint32_t words = (uint32_t)(T.row_bytes >> 2);
    const int64_t nout = nA + nB + 2 * nC;
    const int64_t total = nout * (int64_t)words;
    const uint32_t* __restrict__ src = static_cast<const uint32_t*>(T.src);
    const uint32_t* __restrict__ child = static_cast<const uint32_t*>(T.child);
    uint32_t* __restrict__ dst = static_cast<uint32_t*>(T.dst);
    const bool small = total <= 0xffffffffll;      // (a 32-bit division serves every model that fits a device)
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = small ? (int64_t)((uint32_t)e / words) : e / (int64_t)words;
        const uint32_t w = (uint32_t)(e - r * words);
        uint32_t value = 0;
        bool bad = false;
        if (r < nA) {
            const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_A * stride + r];
            if (srow >= 0 && srow < N) value = src[srow * words + w]; else bad = true;
        } else if (T.kind == GSR_RESIZE_MOMENT) {
            value = 0;                                  // a new Gaussian starts with zero moments: nothing is read
        } else if (r < nA + nB) {
            const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_B * stride + (r - nA)];
            if (srow >= 0 && srow < N) value = src[srow * words + w]; else bad = true;
        } else {
            const int64_t q = r - nA - nB;
            const int64_t copy = q >= nC ? 1 : 0, j = q - copy * nC;      // j < nC <= nSplit <= N: inside the segment
            if (T.kind == GSR_RESIZE_CHILD_SOURCED) {
                const int64_t rank = plan[GSR_RESIZE_PLAN_RANK_C * stride + j];
                if (rank >= 0 && rank < nSplit) value = child[(copy * nSplit + rank) * words + w]; else bad = true;
            } else {
                const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_C * stride + j];
                if (srow >= 0 && srow < N) value = src[srow * words + w]; else bad = true;
            }
        }
        dst[e] = value;
        if (bad && w == 0) atomicOr(reinterpret_cast<unsigned long long*>(meta + GSR_RESIZE_META_STATUS), 1ull);
    }
}

struct MergeTable {
    GsrMergeTensor t[GSR_RESIZE_MAX_TENSORS];
};

// gsr_merge_apply: grid (x, count) as k_resize_apply.  Destination rows [0, nA) are the rows of model a that its plan's A list names, rows
// [nA, nA + nB) those of model b; a MOMENT tensor's b rows are zero and nothing of b is read for them.
__global__ __launch_bounds__(256) void k_merge_apply(const int32_t* __restrict__ rows_a, int64_t Na, int64_t nA, const int32_t* __restrict__ rows_b,
                                                     int64_t Nb, int64_t nB, MergeTable table, int64_t* __restrict__ meta)
{
    const GsrMergeTensor T = table.t[blockIdx.y];
    if (!T.dst || T.row_bytes <= 0) return;
    const uint32_t words = (uint32_t)(T.row_bytes >> 2);
    const int64_t total = (nA + nB) * (int64_t)words;
    const uint32_t* __restrict__ src_a = static_cast<const uint32_t*>(T.src_a);
    const uint32_t* __restrict__ src_b = static_cast<const uint32_t*>(T.src_b);
    uint32_t* __restrict__ dst = static_cast<uint32_t*>(T.dst);
    const bool small = total <= 0xffffffffll;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = small ? (int64_t)((uint32_t)e / words) : e / (int64_t)words;
        const uint32_t w = (uint32_t)(e - r * words);
        uint32_t value = 0;
        bool bad = false;
        if (r < nA) {
            const int64_t srow = rows_a[r];                     // r < nA <= Na: inside the segment
            if (srow >= 0 && srow < Na) value = src_a[srow * words + w]; else bad = true;
        } else if (T.kind != GSR_RESIZE_MOMENT) {
            const int64_t srow = rows_b[r - nA];                // r - nA < nB <= Nb
            if (srow >= 0 && srow < Nb) value = src_b[srow * words + w]; else bad = true;
        }
        dst[e] = value;
        if (bad && w == 0) atomicOr(reinterpret_cast<unsigned long long*>(meta + GSR_RESIZE_META_STATUS), 1ull);
    }
}

// ---- the models of a batch (version 122) -----------------------------------------------------------------------------------------------
// A model starts at a multiple of kBatchBlock = 128 rows, so the plan's 256-row tile could hold the end of one model and the start of the
// next.  The batched plan therefore counts, scans and writes per 128-row block: a block belongs to exactly one model.  The model of a block
// is found from values that are uniform over the workgroup (the block number and the kernel's own arguments), with constant indices into
// the argument tables, so it costs a few scalar selects per block and nothing per row.
constexpr int kBatchBlock = GSR_RESIZE_BLOCK;

struct ResizeBatchDev {
    int32_t B;
    int32_t first_block[GSR_RESIZE_MAX_MODELS + 1];
    int32_t counts[GSR_RESIZE_MAX_MODELS];
};

struct ResizeApplyBatchDev {
    int32_t B;
    int32_t old_first_block[GSR_RESIZE_MAX_MODELS + 1];
    int32_t old_counts[GSR_RESIZE_MAX_MODELS];
    int32_t new_first_block[GSR_RESIZE_MAX_MODELS + 1];
    int32_t c4[GSR_RESIZE_MAX_MODELS][4];                 // nA, nB, nC, nSplit
    int64_t child_base[GSR_RESIZE_MAX_MODELS];            // 2 * sum_{j<b} nSplit_j
};

struct ResizeBatchTable {
    GsrResizeBatchTensor t[GSR_RESIZE_MAX_TENSORS];
};

// inclusive scan over the 128 threads of a workgroup (resize_block_scan for the 128-row block)
__device__ __forceinline__ unsigned long long resize_block_scan128(unsigned long long v, unsigned long long* __restrict__ s, unsigned long long* total)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (unsigned int off = 1; off < (unsigned)kBatchBlock; off <<= 1) {
        const unsigned long long add = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long incl = s[threadIdx.x];
    *total = s[kBatchBlock - 1];
    __syncthreads();
    return incl - v;
}

// the model that owns block `blk` (blk < first_block[B]): the last model whose first block is not beyond it (models without blocks are
// passed over, because a later model starts at the same block); *lo its first block, *cnt its number of rows
__device__ __forceinline__ int resize_batch_model(const ResizeBatchDev& bt, int32_t blk, int32_t* lo, int32_t* cnt)
{
    int b = 0;
    *lo = bt.first_block[0];
    *cnt = bt.counts[0];
#pragma unroll
    for (int j = 1; j < GSR_RESIZE_MAX_MODELS; j++)
        if (j < bt.B && blk >= bt.first_block[j]) { b = j; *lo = bt.first_block[j]; *cnt = bt.counts[j]; }
    return b;
}

// one workgroup of 128 threads per block; tile_count: [4][nblocks]
__global__ __launch_bounds__(128) void k_resize_count_batched(const uint8_t* __restrict__ flags, ResizeBatchDev bt, int64_t nblocks,
                                                              unsigned int* __restrict__ tile_count)
{
    __shared__ unsigned long long s[kBatchBlock];
    int32_t lo, cnt;
    resize_batch_model(bt, (int32_t)blockIdx.x, &lo, &cnt);
    const int64_t i = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const int64_t local = i - (int64_t)lo * kBatchBlock;
    const unsigned long long v = local < cnt ? resize_fields(flags[i]) : 0ull;          // i < 128 * nblocks = N; a padding row counts nowhere
    unsigned long long total;
    resize_block_scan128(v, s, &total);
    if (threadIdx.x < 4) tile_count[(int64_t)threadIdx.x * nblocks + blockIdx.x] = (unsigned int)((total >> (16 * threadIdx.x)) & 0xffffull);
}

// grid (4, B): workgroup (l, b) scans list l's block counts over model b's blocks in place and writes the list's length to meta[b][l];
// workgroup (0, b) also clears the status words of row b
__global__ __launch_bounds__(256) void k_resize_scan_batched(unsigned int* __restrict__ tile_count, ResizeBatchDev bt, int64_t nblocks,
                                                             int64_t* __restrict__ meta)
{
    __shared__ unsigned int s[256];
    int32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < GSR_RESIZE_MAX_MODELS; j++)
        if (j == (int)blockIdx.y) { lo = bt.first_block[j]; hi = bt.first_block[j + 1]; }
    unsigned int* tc = tile_count + (int64_t)blockIdx.x * nblocks;
    unsigned int running = 0;
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t t = base + threadIdx.x;
        const unsigned int v = t < hi ? tc[t] : 0u;
        unsigned int total;
        const unsigned int excl = resize_block_scan(v, s, &total);
        if (t < hi) tc[t] = running + excl;
        running += total;
    }
    int64_t* row = meta + (int64_t)blockIdx.y * GSR_RESIZE_META_WORDS;
    if (threadIdx.x == 0) row[blockIdx.x] = (int64_t)running;
    if (blockIdx.x == 0 && threadIdx.x >= 4 && threadIdx.x < GSR_RESIZE_META_WORDS) row[threadIdx.x] = 0;
}

// the block again: a row's position inside its model's lists = the block's offset in the model + its rank in the block; the list of model b
// starts at entry 128 * first_block[b] of its segment.  Row numbers are store rows, split ranks model-local.
__global__ __launch_bounds__(128) void k_resize_write_batched(const uint8_t* __restrict__ flags, ResizeBatchDev bt, int64_t nblocks,
                                                              const unsigned int* __restrict__ tile_offset, int32_t* __restrict__ plan,
                                                              int64_t stride)
{
    __shared__ unsigned long long s[kBatchBlock];
    int32_t lo, cnt;
    resize_batch_model(bt, (int32_t)blockIdx.x, &lo, &cnt);
    const int64_t i = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const int64_t base = (int64_t)lo * kBatchBlock;
    const bool own = i - base < cnt;
    const unsigned long long v = own ? resize_fields(flags[i]) : 0ull;
    unsigned long long total;
    const unsigned long long excl = resize_block_scan128(v, s, &total);
    if (!own) return;
    const unsigned int pa = tile_offset[blockIdx.x] + (unsigned int)(excl & 0xffffull);
    const unsigned int pb = tile_offset[nblocks + blockIdx.x] + (unsigned int)((excl >> 16) & 0xffffull);
    const unsigned int pc = tile_offset[2 * nblocks + blockIdx.x] + (unsigned int)((excl >> 32) & 0xffffull);
    const unsigned int ps = tile_offset[3 * nblocks + blockIdx.x] + (unsigned int)((excl >> 48) & 0xffffull);
    // a position is below the model's row count (a list holds each of the model's rows at most once), so base + position stays inside the
    // model's blocks of the segment; the comparisons keep a caller's race on the flag bytes inside them as well
    const unsigned int n = (unsigned int)cnt;
    if ((v & 0xffffull) && pa < n) plan[GSR_RESIZE_PLAN_ROWS_A * stride + base + pa] = (int32_t)i;
    if (((v >> 16) & 0xffffull) && pb < n) plan[GSR_RESIZE_PLAN_ROWS_B * stride + base + pb] = (int32_t)i;
    if (((v >> 32) & 0xffffull) && pc < n) {
        plan[GSR_RESIZE_PLAN_ROWS_C * stride + base + pc] = (int32_t)i;
        plan[GSR_RESIZE_PLAN_RANK_C * stride + base + pc] = (int32_t)ps;
    }
    if (((v >> 48) & 0xffffull) && ps < n) plan[GSR_RESIZE_PLAN_SPLIT_ROWS * stride + base + ps] = (int32_t)i;
}

__global__ void k_resize_meta_zero_batched(int64_t* __restrict__ meta, int words)
{
    if ((int)threadIdx.x < words) meta[threadIdx.x] = 0;
}

// grid (x, count): tensor blockIdx.y; the x dimension strides over the 128-row blocks of the NEW store, the threads over a block's words,
// so a wave stores 256 consecutive bytes.  The model of a block is uniform over the workgroup.
__global__ __launch_bounds__(256) void k_resize_apply_batched(const int32_t* __restrict__ plan, int64_t stride, ResizeApplyBatchDev bt,
                                                              int32_t nblocks, ResizeBatchTable table, int64_t* __restrict__ meta)
{
    const GsrResizeBatchTensor T = table.t[blockIdx.y];
    if (!T.src || !T.dst || T.row_bytes <= 0) return;
    const uint32_t words = (uint32_t)(T.row_bytes >> 2);
    const uint32_t* __restrict__ src = static_cast<const uint32_t*>(T.src);
    const uint32_t* __restrict__ child = static_cast<const uint32_t*>(T.child);
    const uint32_t* __restrict__ pad = static_cast<const uint32_t*>(T.pad);
    uint32_t* __restrict__ dst = static_cast<uint32_t*>(T.dst);
    const int64_t per_block = (int64_t)kBatchBlock * words;
    const bool small = per_block <= 0xffffffffll;
    for (int32_t blk = (int32_t)blockIdx.x; blk < nblocks; blk += (int32_t)gridDim.x) {
        // the model of this block of the new store, and what the rows of that model need (all uniform)
        int b = 0;
        int32_t new_lo = bt.new_first_block[0], old_lo = bt.old_first_block[0], old_cnt = bt.old_counts[0];
        int32_t cA = bt.c4[0][0], cB = bt.c4[0][1], cC = bt.c4[0][2], cS = bt.c4[0][3];
        int64_t child_base = bt.child_base[0];
#pragma unroll
        for (int j = 1; j < GSR_RESIZE_MAX_MODELS; j++)
            if (j < bt.B && blk >= bt.new_first_block[j]) {
                b = j; new_lo = bt.new_first_block[j]; old_lo = bt.old_first_block[j]; old_cnt = bt.old_counts[j];
                cA = bt.c4[j][0]; cB = bt.c4[j][1]; cC = bt.c4[j][2]; cS = bt.c4[j][3]; child_base = bt.child_base[j];
            }
        const int64_t nA = cA, nB = cB, nC = cC, nSplit = cS, nout = nA + nB + 2 * nC;
        const int64_t seg = (int64_t)old_lo * kBatchBlock;                  // the model's first entry in every segment = its first old store row
        const int64_t row_lo = seg, row_hi = seg + old_cnt;                  // the model's own rows of the old store
        const int64_t r0 = ((int64_t)blk - new_lo) * kBatchBlock;            // the block's first row inside the model's new rows
        const int64_t e0 = (int64_t)blk * per_block;
        for (int64_t k = threadIdx.x; k < per_block; k += 256) {
            const int64_t rl = small ? (int64_t)((uint32_t)k / words) : k / (int64_t)words;
            const uint32_t w = (uint32_t)(k - rl * words);
            const int64_t r = r0 + rl;
            uint32_t value = 0;
            bool bad = false;
            if (r >= nout) {
                value = (T.kind != GSR_RESIZE_MOMENT && pad) ? pad[w] : 0u;      // padding
            } else if (r < nA) {
                const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_A * stride + seg + r];      // r < nA <= counts[b]: inside the model's blocks
                if (srow >= row_lo && srow < row_hi) value = src[srow * words + w]; else bad = true;
            } else if (T.kind == GSR_RESIZE_MOMENT) {
                value = 0;
            } else if (r < nA + nB) {
                const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_B * stride + seg + (r - nA)];
                if (srow >= row_lo && srow < row_hi) value = src[srow * words + w]; else bad = true;
            } else {
                const int64_t q = r - nA - nB;
                const int64_t copy = q >= nC ? 1 : 0, j = q - copy * nC;          // j < nC <= nSplit <= counts[b]
                if (T.kind == GSR_RESIZE_CHILD_SOURCED) {
                    const int64_t rank = plan[GSR_RESIZE_PLAN_RANK_C * stride + seg + j];
                    if (rank >= 0 && rank < nSplit) value = child[(child_base + copy * nSplit + rank) * words + w]; else bad = true;
                } else {
                    const int64_t srow = plan[GSR_RESIZE_PLAN_ROWS_C * stride + seg + j];
                    if (srow >= row_lo && srow < row_hi) value = src[srow * words + w]; else bad = true;
                }
            }
            dst[e0 + k] = value;
            if (bad && w == 0)
                atomicOr(reinterpret_cast<unsigned long long*>(meta + (int64_t)b * GSR_RESIZE_META_WORDS + GSR_RESIZE_META_STATUS), 1ull);
        }
    }
}

static inline int64_t resize_stride(int64_t N) { return (N + 63) / 64 * 64; }      // entries per plan segment: 256-byte aligned segments
static inline int64_t resize_tiles(int64_t N) { return (N + kResizeTile - 1) / kResizeTile; }

// the rules of a GsrResizeBatch; *N = 128 * first_block[B]
static int resize_check_batch(const char* who, const GsrResizeBatch* batch, int64_t* N)
{
    char text[256];
    auto refuse = [&](const char* rule) { snprintf(text, sizeof text, "%s: %s", who, rule); return fail_text(GSR_ERR_ARG, text); };
    if (!batch) return refuse("batch is NULL");
    if (batch->B < 1 || batch->B > GSR_RESIZE_MAX_MODELS) return refuse("B must be in [1, GSR_RESIZE_MAX_MODELS] (16)");
    if (batch->first_block[0] != 0) return refuse("first_block must start at 0");
    for (int b = 0; b < batch->B; b++) {
        if (batch->first_block[b + 1] < batch->first_block[b]) return refuse("first_block must not decrease");
        if (batch->first_block[b + 1] >= ((int64_t)1 << 31) / kBatchBlock) return refuse("N = 128 * first_block[B] must be below 2^31");
        if (batch->counts[b] < 0 || batch->counts[b] > (batch->first_block[b + 1] - batch->first_block[b]) * kBatchBlock)
            return refuse("counts[b] must be in [0, 128 * (first_block[b + 1] - first_block[b])]: a model's rows lie inside its blocks");
    }
    *N = batch->first_block[batch->B] * kBatchBlock;
    return GSR_OK;
}

static ResizeBatchDev resize_batch_dev(const GsrResizeBatch* batch)
{
    ResizeBatchDev d{};
    d.B = batch->B;
    for (int b = 0; b <= GSR_RESIZE_MAX_MODELS; b++) d.first_block[b] = (int32_t)batch->first_block[b <= batch->B ? b : batch->B];
    for (int b = 0; b < batch->B; b++) d.counts[b] = (int32_t)batch->counts[b];
    return d;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_resize_scratch_bytes(int64_t N)
{
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) N = ((int64_t)1 << 31) - 1;      // (larger models are refused by the call itself)
    return ((size_t)resize_tiles(N) * 4 * sizeof(unsigned int) + 255) & ~(size_t)255;
}

size_t gsr_resize_plan_bytes(int64_t N)
{
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) N = ((int64_t)1 << 31) - 1;
    return (size_t)resize_stride(N) * GSR_RESIZE_PLAN_SEGMENTS * sizeof(int32_t);
}

int gsr_resize_plan(const uint8_t* flags, int64_t N, void* plan, size_t plan_bytes, int64_t* meta, void* scratch, size_t scratch_bytes,
                    void* stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31)) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: N must be in [0, 2^31)");
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: meta is NULL or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        hipLaunchKernelGGL(k_resize_meta_zero, dim3(1), dim3(64), 0, st, meta);
        return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
    }
    if (!flags) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: flags is NULL");
    if (!plan || ((uintptr_t)plan & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: plan is NULL or not 4-byte aligned");
    if (plan_bytes < gsr_resize_plan_bytes(N)) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: plan is shorter than gsr_resize_plan_bytes(N)");
    if (!scratch || ((uintptr_t)scratch & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan: scratch is NULL or not 4-byte aligned");
    if (scratch_bytes < gsr_resize_scratch_bytes(N))
        return fail_text(GSR_ERR_ARG, "gsr_resize_plan: scratch is shorter than gsr_resize_scratch_bytes(N)");
    const int64_t ntiles = resize_tiles(N), stride = resize_stride(N);
    unsigned int* tiles = static_cast<unsigned int*>(scratch);
    hipLaunchKernelGGL(k_resize_count, dim3((unsigned)ntiles), dim3(256), 0, st, flags, N, ntiles, tiles);
    hipLaunchKernelGGL(k_resize_scan_tiles, dim3(4), dim3(256), 0, st, tiles, ntiles, meta);
    hipLaunchKernelGGL(k_resize_write, dim3((unsigned)ntiles), dim3(256), 0, st, flags, N, ntiles, tiles, static_cast<int32_t*>(plan), stride);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_resize_apply(const void* plan, size_t plan_bytes, int64_t N, int64_t nA, int64_t nB, int64_t nC, int64_t nSplit,
                     const GsrResizeTensor* tensors, int32_t count, int64_t* meta, void* stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31)) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: N must be in [0, 2^31)");
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: meta is NULL or not 8-byte aligned");
    if (count < 0 || count > GSR_RESIZE_MAX_TENSORS) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: at most GSR_RESIZE_MAX_TENSORS (18) tensors");
    if (count > 0 && !tensors) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: tensors is NULL");
    if (nA < 0 || nB < 0 || nC < 0 || nSplit < 0 || nA > N || nB > N || nSplit > N || nC > nSplit)
        return fail_text(GSR_ERR_ARG, "gsr_resize_apply: counts beyond the plan's capacity (0 <= nA, nB, nSplit <= N and nC <= nSplit)");
    const int64_t nout = nA + nB + 2 * nC;
    if (nout > 0 && (!plan || ((uintptr_t)plan & 3) != 0)) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: plan is NULL or not 4-byte aligned");
    if (nout > 0 && plan_bytes < gsr_resize_plan_bytes(N))
        return fail_text(GSR_ERR_ARG, "gsr_resize_apply: plan is shorter than gsr_resize_plan_bytes(N)");
    ResizeTable table{};
    int64_t most = 0;
    for (int k = 0; k < count; k++) {
        const GsrResizeTensor& t = tensors[k];
        if (t.row_bytes < 0 || (t.row_bytes & 3) != 0 || t.row_bytes >= ((int64_t)1 << 31))
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply: row_bytes must be a non-negative multiple of 4 below 2^31");
        if (t.kind != GSR_RESIZE_PARAM && t.kind != GSR_RESIZE_MOMENT && t.kind != GSR_RESIZE_CHILD_SOURCED)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply: kind is GSR_RESIZE_PARAM, GSR_RESIZE_MOMENT or GSR_RESIZE_CHILD_SOURCED");
        table.t[k] = t;
        if (t.row_bytes == 0 || (!t.src && !t.dst)) { table.t[k].src = nullptr; table.t[k].dst = nullptr; continue; }      // skipped
        if (!t.src || !t.dst) return fail_text(GSR_ERR_ARG, "gsr_resize_apply: src and dst are given both or neither");
        if ((((uintptr_t)t.src | (uintptr_t)t.dst | (uintptr_t)t.child) & 3) != 0)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply: src, dst and child must be 4-byte aligned");
        if (t.kind == GSR_RESIZE_CHILD_SOURCED && nC > 0 && !t.child)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply: a GSR_RESIZE_CHILD_SOURCED tensor needs child rows when nC > 0");
        const int64_t words = nout * (t.row_bytes >> 2);
        if (words > most) most = words;
    }
    if (most == 0) return GSR_OK;      // nothing kept, or nothing to move: not an error
    int64_t gx = (most + 255) / 256;
    if (gx > kResizeApplyGridX) gx = kResizeApplyGridX;
    hipLaunchKernelGGL(k_resize_apply, dim3((unsigned)gx, (unsigned)count), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const int32_t*>(plan), resize_stride(N), N, nA, nB, nC, nSplit, table, meta);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

size_t gsr_resize_scratch_bytes_batched(int64_t N)
{
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) N = ((int64_t)1 << 31) - 1;      // (larger stores are refused by the call itself)
    return ((size_t)((N + kBatchBlock - 1) / kBatchBlock) * 4 * sizeof(unsigned int) + 255) & ~(size_t)255;
}

int gsr_resize_plan_batched(const uint8_t* flags, const GsrResizeBatch* batch, void* plan, size_t plan_bytes, int64_t* meta, void* scratch,
                            size_t scratch_bytes, void* stream)
{
    int64_t N = 0;
    if (resize_check_batch("gsr_resize_plan_batched", batch, &N) != GSR_OK) return GSR_ERR_ARG;
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: meta is NULL or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        hipLaunchKernelGGL(k_resize_meta_zero_batched, dim3(1), dim3(GSR_RESIZE_MAX_MODELS * GSR_RESIZE_META_WORDS), 0, st, meta,
                           batch->B * GSR_RESIZE_META_WORDS);
        return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
    }
    if (!flags) return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: flags is NULL");
    if (!plan || ((uintptr_t)plan & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: plan is NULL or not 4-byte aligned");
    if (plan_bytes < gsr_resize_plan_bytes(N))
        return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: plan is shorter than gsr_resize_plan_bytes(N)");
    if (!scratch || ((uintptr_t)scratch & 3) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: scratch is NULL or not 4-byte aligned");
    if (scratch_bytes < gsr_resize_scratch_bytes_batched(N))
        return fail_text(GSR_ERR_ARG, "gsr_resize_plan_batched: scratch is shorter than gsr_resize_scratch_bytes_batched(N)");
    const int64_t nblocks = N / kBatchBlock, stride = resize_stride(N);
    const ResizeBatchDev bt = resize_batch_dev(batch);
    unsigned int* tiles = static_cast<unsigned int*>(scratch);
    hipLaunchKernelGGL(k_resize_count_batched, dim3((unsigned)nblocks), dim3(kBatchBlock), 0, st, flags, bt, nblocks, tiles);
    hipLaunchKernelGGL(k_resize_scan_batched, dim3(4, (unsigned)batch->B), dim3(256), 0, st, tiles, bt, nblocks, meta);
    hipLaunchKernelGGL(k_resize_write_batched, dim3((unsigned)nblocks), dim3(kBatchBlock), 0, st, flags, bt, nblocks, tiles,
                       static_cast<int32_t*>(plan), stride);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_resize_apply_batched(const void* plan, size_t plan_bytes, const GsrResizeBatch* old_batch, const int64_t* counts4,
                             const int64_t* new_first_block, const GsrResizeBatchTensor* tensors, int32_t count, int64_t* meta, void* stream)
{
    int64_t N = 0;
    if (resize_check_batch("gsr_resize_apply_batched", old_batch, &N) != GSR_OK) return GSR_ERR_ARG;
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: meta is NULL or not 8-byte aligned");
    if (!counts4) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: counts4 is NULL");
    if (!new_first_block) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: new_first_block is NULL");
    if (count < 0 || count > GSR_RESIZE_MAX_TENSORS)
        return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: at most GSR_RESIZE_MAX_TENSORS (18) tensors");
    if (count > 0 && !tensors) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: tensors is NULL");
    const int B = old_batch->B;
    ResizeApplyBatchDev bt{};
    bt.B = B;
    int64_t kept = 0, children = 0, with_children = 0, next_block = 0;
    if (new_first_block[0] != 0) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: new_first_block must start at 0");
    for (int b = 0; b < B; b++) {
        const int64_t nA = counts4[4 * b], nB = counts4[4 * b + 1], nC = counts4[4 * b + 2], nS = counts4[4 * b + 3], cap = old_batch->counts[b];
        if (nA < 0 || nB < 0 || nC < 0 || nS < 0 || nA > cap || nB > cap || nS > cap || nC > nS)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: counts beyond a model's capacity (0 <= nA, nB, nSplit <= counts[b] and nC <= nSplit)");
        const int64_t nout = nA + nB + 2 * nC;
        const int64_t blocks = nout == 0 ? 1 : (nout + kBatchBlock - 1) / kBatchBlock;
        next_block += blocks;
        if (new_first_block[b + 1] != next_block)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: new_first_block[b + 1] - new_first_block[b] must be max(1, ceil((nA + nB + 2 nC) / 128)) "
                                          "of model b");
        if (next_block >= ((int64_t)1 << 31) / kBatchBlock)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: the new store, 128 * new_first_block[B] rows, must be below 2^31 rows");
        bt.old_first_block[b] = (int32_t)old_batch->first_block[b];
        bt.old_counts[b] = (int32_t)cap;
        bt.new_first_block[b] = (int32_t)new_first_block[b];
        bt.c4[b][0] = (int32_t)nA; bt.c4[b][1] = (int32_t)nB; bt.c4[b][2] = (int32_t)nC; bt.c4[b][3] = (int32_t)nS;
        bt.child_base[b] = 2 * children;
        children += nS;
        kept += nout;
        with_children += nC;
    }
    for (int b = B; b <= GSR_RESIZE_MAX_MODELS; b++) {
        bt.old_first_block[b] = (int32_t)old_batch->first_block[B];
        bt.new_first_block[b] = (int32_t)next_block;
    }
    if (kept > 0 && (!plan || ((uintptr_t)plan & 3) != 0)) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: plan is NULL or not 4-byte aligned");
    if (kept > 0 && plan_bytes < gsr_resize_plan_bytes(N))
        return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: plan is shorter than gsr_resize_plan_bytes(N)");
    ResizeBatchTable table{};
    bool moves = false;
    for (int k = 0; k < count; k++) {
        const GsrResizeBatchTensor& t = tensors[k];
        if (t.row_bytes < 0 || (t.row_bytes & 3) != 0 || t.row_bytes >= ((int64_t)1 << 31))
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: row_bytes must be a non-negative multiple of 4 below 2^31");
        if (t.kind != GSR_RESIZE_PARAM && t.kind != GSR_RESIZE_MOMENT && t.kind != GSR_RESIZE_CHILD_SOURCED)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: kind is GSR_RESIZE_PARAM, GSR_RESIZE_MOMENT or GSR_RESIZE_CHILD_SOURCED");
        table.t[k] = t;
        if (t.row_bytes == 0 || (!t.src && !t.dst)) { table.t[k].src = nullptr; table.t[k].dst = nullptr; continue; }      // skipped
        if (!t.src || !t.dst) return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: src and dst are given both or neither");
        if ((((uintptr_t)t.src | (uintptr_t)t.dst | (uintptr_t)t.child | (uintptr_t)t.pad) & 3) != 0)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: src, dst, child and pad must be 4-byte aligned");
        if (t.kind == GSR_RESIZE_CHILD_SOURCED && with_children > 0 && !t.child)
            return fail_text(GSR_ERR_ARG, "gsr_resize_apply_batched: a GSR_RESIZE_CHILD_SOURCED tensor needs child rows when a model's nC > 0");
        moves = true;
    }
    if (!moves) return GSR_OK;      // nothing to write: not an error
    int64_t gx = next_block;        // (every model keeps a block, so the new store is never empty)
    if (gx > kResizeApplyGridX) gx = kResizeApplyGridX;
    hipLaunchKernelGGL(k_resize_apply_batched, dim3((unsigned)gx, (unsigned)count), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const int32_t*>(plan), resize_stride(N), bt, (int32_t)next_block, table, meta);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_merge_apply(const void* plan_a, size_t plan_a_bytes, int64_t Na, int64_t nA, const void* plan_b, size_t plan_b_bytes, int64_t Nb, int64_t nB,
                    const GsrMergeTensor* tensors, int32_t count, int64_t* meta, void* stream)
{
    if (Na < 0 || Na >= ((int64_t)1 << 31) || Nb < 0 || Nb >= ((int64_t)1 << 31))
        return fail_text(GSR_ERR_ARG, "gsr_merge_apply: Na and Nb must be in [0, 2^31)");
    if (!meta || ((uintptr_t)meta & 7) != 0) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: meta is NULL or not 8-byte aligned");
    if (count < 0 || count > GSR_RESIZE_MAX_TENSORS) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: at most GSR_RESIZE_MAX_TENSORS (18) tensors");
    if (count > 0 && !tensors) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: tensors is NULL");
    if (nA < 0 || nB < 0 || nA > Na || nB > Nb)
        return fail_text(GSR_ERR_ARG, "gsr_merge_apply: counts beyond the plans' capacity (0 <= nA <= Na and 0 <= nB <= Nb)");
    if (nA > 0 && (!plan_a || ((uintptr_t)plan_a & 3) != 0)) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: plan_a is NULL or not 4-byte aligned");
    if (nA > 0 && plan_a_bytes < gsr_resize_plan_bytes(Na)) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: plan_a is shorter than gsr_resize_plan_bytes(Na)");
    if (nB > 0 && (!plan_b || ((uintptr_t)plan_b & 3) != 0)) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: plan_b is NULL or not 4-byte aligned");
    if (nB > 0 && plan_b_bytes < gsr_resize_plan_bytes(Nb)) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: plan_b is shorter than gsr_resize_plan_bytes(Nb)");
    MergeTable table{};
    int64_t most = 0;
    for (int k = 0; k < count; k++) {
        const GsrMergeTensor& t = tensors[k];
        if (t.row_bytes < 0 || (t.row_bytes & 3) != 0 || t.row_bytes >= ((int64_t)1 << 31))
            return fail_text(GSR_ERR_ARG, "gsr_merge_apply: row_bytes must be a non-negative multiple of 4 below 2^31");
        if (t.kind != GSR_RESIZE_PARAM && t.kind != GSR_RESIZE_MOMENT)
            return fail_text(GSR_ERR_ARG, "gsr_merge_apply: kind is GSR_RESIZE_PARAM or GSR_RESIZE_MOMENT");
        table.t[k] = t;
        if (t.row_bytes == 0 || (!t.src_a && !t.src_b && !t.dst)) { table.t[k].dst = nullptr; continue; }      // skipped
        if (!t.dst) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: dst is NULL for a tensor with sources");
        if (nA > 0 && !t.src_a) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: src_a is NULL when nA > 0");
        if (nB > 0 && t.kind == GSR_RESIZE_PARAM && !t.src_b) return fail_text(GSR_ERR_ARG, "gsr_merge_apply: src_b is NULL for a GSR_RESIZE_PARAM tensor when nB > 0");
        if ((((uintptr_t)t.src_a | (uintptr_t)t.src_b | (uintptr_t)t.dst) & 3) != 0)
            return fail_text(GSR_ERR_ARG, "gsr_merge_apply: src_a, src_b and dst must be 4-byte aligned");
        const int64_t words = (nA + nB) * (t.row_bytes >> 2);
        if (words > most) most = words;
    }
    if (most == 0) return GSR_OK;      // nothing kept, or nothing to move: not an error
    int64_t gx = (most + 255) / 256;
    if (gx > kResizeApplyGridX) gx = kResizeApplyGridX;
    const int32_t* rows_a = plan_a ? static_cast<const int32_t*>(plan_a) + GSR_RESIZE_PLAN_ROWS_A * resize_stride(Na) : nullptr;
    const int32_t* rows_b = plan_b ? static_cast<const int32_t*>(plan_b) + GSR_RESIZE_PLAN_ROWS_A * resize_stride(Nb) : nullptr;
    hipLaunchKernelGGL(k_merge_apply, dim3((unsigned)gx, (unsigned)count), dim3(256), 0, (hipStream_t)stream, rows_a, Na, nA, rows_b, Nb, nB, table, meta);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
