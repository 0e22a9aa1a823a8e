// K13 of SURVEY §2b: device-side slice pack for Federation.distribute
// (reference hot site: src/fed.py:161-178, host deepcopies per client).
// Every dense-prefix slice is a (rows, cols) strided 2-D copy out of the
// global master tensor; ONE kernel launch copies every client's every
// slice from a descriptor table instead of ~600 narrow+clone launches per
// round.  Descriptors and destination buffers are cached per rate
// assignment (pointers are stable: global params update in place).
#include "common.h"

struct PackSpan {
    const float* src;
    float* dst;
    int rows;
    int cols;
    int src_stride;
    int pad;
};

__global__ void __launch_bounds__(256)
pack_slices_kernel(const PackSpan* __restrict__ spans, int n,
                   int rows_per_block) {
    const int d = blockIdx.x;
    if (d >= n) return;
    const PackSpan sp = spans[d];
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(sp.rows, r0 + rows_per_block);
    for (int r = r0; r < r1; ++r) {
        const float* s = sp.src + (long)r * sp.src_stride;
        float* t = sp.dst + (long)r * sp.cols;
        for (int c = threadIdx.x; c < sp.cols; c += blockDim.x)
            t[c] = s[c];
    }
}

// Rolled / per-head slices (cfg submodel = 'roll'): each axis of a slice is
// a periodic window {size, period, shift, take}; local index j maps to
// global index (j / take) * period + (shift + j % take) % period.  FULL is
// {size, size, 0, size}, PREFIX(n) {size, size, 0, n}, ROLL(n, shift)
// {size, size, shift, n}, and the transformer's per-head q/k/v slice
// {size, head_dim, shift % head_dim, local_hd}.
struct PackWindow {
    int size;
    int period;
    int shift;
    int take;
};

__device__ __forceinline__ int window_global(const PackWindow& w, int j) {
    const int q = j / w.take;
    int g = w.shift + (j - q * w.take);
    if (g >= w.period) g -= w.period;   // shift < period, j % take < period
    return q * w.period + g;
}

// dst[r, c, t] = src[g_out(r), g_in(c), t]; a 1-D tensor is rows = 1 with
// its axis as `in`.
struct RollSpan {
    const float* src;
    float* dst;
    PackWindow out;
    PackWindow in;
    int rows;            // local out size
    int cols;            // local in size
    int inner;           // kh * kw (1 for linear weights)
    int rows_per_block;
};

// blocks[b] = {span, first row}: one block copies rows_per_block local rows
__global__ void __launch_bounds__(256)
pack_slices_roll_kernel(const RollSpan* __restrict__ spans,
                        const int2* __restrict__ blocks, int n_blocks) {
    if ((int)blockIdx.x >= n_blocks) return;
    const int2 b = blocks[blockIdx.x];
    const RollSpan sp = spans[b.x];
    const int r1 = min(sp.rows, b.y + sp.rows_per_block);
    const int width = sp.cols * sp.inner;
    const long src_row = (long)sp.in.size * sp.inner;
    for (int r = b.y; r < r1; ++r) {
        const float* s = sp.src + (long)window_global(sp.out, r) * src_row;
        float* t = sp.dst + (long)r * width;
        for (int x = threadIdx.x; x < width; x += blockDim.x) {
            const int c = x / sp.inner;
            const int k = x - c * sp.inner;
            t[x] = s[(long)window_global(sp.in, c) * sp.inner + k];
        }
    }
}

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

void pack_slices(at::Tensor blob, int64_t n, int64_t max_rows) {
    TORCH_CHECK(blob.is_cuda() && blob.is_contiguous());
    const int rpb = 16;
    const int ny = (int)((max_rows + rpb - 1) / rpb);
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pack_slices_kernel, dim3((unsigned)n, ny), dim3(256),
                       0, stream, (const PackSpan*)blob.data_ptr(), (int)n,
                       rpb);
}

void pack_slices_roll(at::Tensor spans, int64_t n_spans, at::Tensor blocks) {
    TORCH_CHECK(spans.is_cuda() && spans.is_contiguous()
                && spans.scalar_type() == at::kByte);
    TORCH_CHECK(blocks.is_cuda() && blocks.is_contiguous()
                && blocks.scalar_type() == at::kInt && blocks.dim() == 2
                && blocks.size(1) == 2);
    static_assert(sizeof(RollSpan) == 64,
                  "span layout is mirrored in fed/federation.py");
    TORCH_CHECK(spans.numel() == n_spans * (int64_t)sizeof(RollSpan),
                "pack_slices_roll: span table size");
    const int64_t n_blocks = blocks.size(0);
    if (n_blocks == 0) return;
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pack_slices_roll_kernel, dim3((unsigned)n_blocks),
                       dim3(256), 0, stream,
                       (const RollSpan*)spans.data_ptr(),
                       (const int2*)blocks.data_ptr(), (int)n_blocks);
}
