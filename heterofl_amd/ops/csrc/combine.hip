// K14 of SURVEY §2b, single-GPU form: the gather form of
// Federation.accumulate.  One lane per GLOBAL element: it walks the reporting
// clients in ascending slot order, inverts each client's slice maps, and adds
// the client's value where the element is a member — no atomics, and the
// same fp32 additions in the same order as the torch loop, so tmp and cnt
// are bit-identical to it.  Elements nobody covers are written as zeros, so
// the accumulators need no memset.
//
// Each axis of a client's slice is a periodic window {period, shift, take}
// over the global axis (see pack.hip): global index g belongs to it iff
// w = (g % period - shift + period) % period < take, at local index
// (g / period) * take + w.
#include "common.h"

struct CombWindow {
    int period;
    int shift;
    int take;
};

// one (tensor, reporting client) pair
struct CombEntry {
    const float* val;           // (n_out, n_in, inner) contiguous
    const unsigned char* mask;  // per local out row, or null: admit all
    CombWindow out;
    CombWindow in;
    int n_in;                   // local in size
    int pad;
};

// one global tensor, viewed as (O, I, inner); 1-D tensors have I = 1
struct CombTensor {
    float* tmp;
    float* cnt;
    int O;
    int I;
    int inner;
    int ent_start;   // first CombEntry; entries are in ascending slot order
    int ent_count;   // 0: nobody reported, tmp = cnt = 0
    int pad;
};

// local index of global index g, or -1 when g is outside the window
__device__ __forceinline__ int window_local(const CombWindow& w, int g) {
    const int q = g / w.period;
    int r = g - q * w.period - w.shift;
    if (r < 0) r += w.period;
    return r < w.take ? q * w.take + r : -1;
}

#define COMB_PER_BLOCK 1024

// blocks[b] = {tensor, first element}: one block owns COMB_PER_BLOCK
// consecutive elements of one tensor
__global__ void __launch_bounds__(256)
combine_accumulate_kernel(const CombTensor* __restrict__ tensors,
                          const CombEntry* __restrict__ entries,
                          const int2* __restrict__ blocks, int n_blocks) {
    if ((int)blockIdx.x >= n_blocks) return;
    const int2 b = blocks[blockIdx.x];
    const CombTensor T = tensors[b.x];
    const long numel = (long)T.O * T.I * T.inner;
    const long e1 = min(numel, (long)b.y + COMB_PER_BLOCK);
    for (long e = (long)b.y + threadIdx.x; e < e1; e += blockDim.x) {
        const int oi = (int)(e / T.inner);
        const int t = (int)(e - (long)oi * T.inner);
        const int o = oi / T.I;
        const int i = oi - o * T.I;
        float acc = 0.f, cnt = 0.f;
        for (int c = 0; c < T.ent_count; ++c) {
            const CombEntry en = entries[T.ent_start + c];
            const int jo = window_local(en.out, o);
            if (jo < 0) continue;
            const int ji = window_local(en.in, i);
            if (ji < 0) continue;
            if (en.mask != nullptr && en.mask[jo] == 0) continue;
            acc += en.val[((long)jo * en.n_in + ji) * T.inner + t];
            cnt += 1.f;
        }
        T.tmp[e] = acc;
        T.cnt[e] = cnt;
    }
}

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

// table: [n_tensors CombTensor | CombEntry ...] as bytes (built by
// ops.fused.combine_accumulate, which validates every shape it points at).
void combine_accumulate(at::Tensor table, int64_t n_tensors,
                        int64_t n_entries, at::Tensor blocks) {
    TORCH_CHECK(table.is_cuda() && table.is_contiguous()
                && table.scalar_type() == at::kByte);
    TORCH_CHECK(blocks.is_cuda() && blocks.is_contiguous()
                && blocks.scalar_type() == at::kInt && blocks.dim() == 2
                && blocks.size(1) == 2);
    static_assert(sizeof(CombTensor) == 40 && sizeof(CombEntry) == 48,
                  "table layout is mirrored in ops/fused.py");
    const int64_t ent_off = n_tensors * (int64_t)sizeof(CombTensor);
    TORCH_CHECK(table.numel() >= ent_off
                + n_entries * (int64_t)sizeof(CombEntry),
                "combine_accumulate: table size");
    const int64_t n_blocks = blocks.size(0);
    if (n_blocks == 0) return;
    auto stream = at::hip::getCurrentHIPStream();
    const char* base = (const char*)table.data_ptr();
    hipLaunchKernelGGL(combine_accumulate_kernel, dim3((unsigned)n_blocks),
                       dim3(256), 0, stream, (const CombTensor*)base,
                       (const CombEntry*)(base + ent_off),
                       (const int2*)blocks.data_ptr(), (int)n_blocks);
}
