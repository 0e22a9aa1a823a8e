// The graphed vision step's batch fetch in one launch: rows
// counter*B .. counter*B + B - 1 of the epoch buffers x_all (cap, ...) and
// y_all (cap, R) into fresh (B, ...) tensors, and counter += 1 for the next
// replay.  Replaces counter*B, + arange, two index_selects and the in-place
// counter add.
//
// Every block reads the old counter before it takes a ticket (a device-scope
// atomic from lane 0, after the block's loads of it are done); the block that
// draws the last ticket writes counter + 1 and puts the ticket word back to 0,
// so nobody can see the new value and a replay needs no host work.  A batch
// that does not lie inside the buffers is not read (index_select would
// fault): xb and yb come back all zero and the counter still advances.
#include "common.h"

template <typename U>
__device__ __forceinline__ void copy_units(const void* src, void* dst,
                                           long units) {
    const U* s = (const U*)src;
    U* d = (U*)dst;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < units;
         i += (long)gridDim.x * blockDim.x)
        d[i] = s[i];
}

template <typename U>
__device__ __forceinline__ void zero_units(void* dst, long units) {
    U* d = (U*)dst;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < units;
         i += (long)gridDim.x * blockDim.x)
        d[i] = U{};
}

// XU: bytes per access for x (16 when rows and bases allow, else its element
// size); y moves as 8-byte labels.
template <int XU>
__global__ void __launch_bounds__(256)
batch_gather_kernel(const char* __restrict__ x_all, const char* __restrict__ y_all,
                    char* __restrict__ xb, char* __restrict__ yb,
                    long* __restrict__ counter, unsigned* __restrict__ ticket,
                    long last, long B, long x_row_bytes, long y_row_bytes) {
    const long cnt = counter[0];
    if (cnt >= 0 && cnt <= last) {   // last = cap / B - 1
        const long row0 = cnt * B;
        const char* xs = x_all + row0 * x_row_bytes;
        const long xbytes = B * x_row_bytes;
        if (XU == 16) copy_units<uint4>(xs, xb, xbytes / 16);
        else if (XU == 8) copy_units<unsigned long>(xs, xb, xbytes / 8);
        else if (XU == 4) copy_units<unsigned>(xs, xb, xbytes / 4);
        else if (XU == 2) copy_units<unsigned short>(xs, xb, xbytes / 2);
        else copy_units<unsigned char>(xs, xb, xbytes);
        copy_units<unsigned long>(y_all + row0 * y_row_bytes, yb,
                                  B * y_row_bytes / 8);
    } else {
        zero_units<unsigned char>(xb, B * x_row_bytes);
        zero_units<unsigned long>(yb, B * y_row_bytes / 8);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned t = atomicAdd(ticket, 1u);
        if (t == gridDim.x - 1) {
            counter[0] = cnt + 1;
            atomicExch(ticket, 0u);
        }
    }
}

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

// x_all (cap, ...), y_all (cap, R) int64, counter (1,) int64, ticket (1,)
// int32 holding 0 -> (xb (B, ...), yb (B, R)); counter is left at counter + 1
std::vector<at::Tensor> batch_gather(at::Tensor x_all, at::Tensor y_all,
                                     at::Tensor counter, at::Tensor ticket,
                                     int64_t B) {
    TORCH_CHECK(x_all.is_cuda() && x_all.is_contiguous() &&
                y_all.is_cuda() && y_all.is_contiguous());
    TORCH_CHECK(y_all.scalar_type() == at::kLong && y_all.dim() == 2);
    TORCH_CHECK(counter.is_cuda() && counter.scalar_type() == at::kLong &&
                counter.numel() == 1);
    TORCH_CHECK(ticket.is_cuda() && ticket.scalar_type() == at::kInt &&
                ticket.numel() == 1);
    const long cap = x_all.size(0);
    TORCH_CHECK(B >= 1 && B <= cap && y_all.size(0) == cap,
                "batch_gather: batch / capacity mismatch");
    auto xs = x_all.sizes().vec();
    xs[0] = B;
    auto xb = at::empty(xs, x_all.options());
    auto yb = at::empty({(long)B, y_all.size(1)}, y_all.options());
    const long esz = x_all.element_size();
    const long x_row_bytes = x_all.numel() / cap * esz;
    const long y_row_bytes = y_all.size(1) * 8;
    const bool vec = x_row_bytes % 16 == 0 &&
                     ptr_aligned(x_all.data_ptr(), 16) &&
                     ptr_aligned(xb.data_ptr(), 16);
    const int xu = vec ? 16 : (int)esz;
    const long units = std::max(B * x_row_bytes / xu, B * y_row_bytes / 8);
    const int grid = (int)std::min<long>(128, std::max<long>(1, (units + 255) / 256));
    auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_BG(XU)                                                         \
    hipLaunchKernelGGL(batch_gather_kernel<XU>, dim3(grid), dim3(256), 0,     \
                       stream, (const char*)x_all.data_ptr(),                 \
                       (const char*)y_all.data_ptr(), (char*)xb.data_ptr(),   \
                       (char*)yb.data_ptr(), (long*)counter.data_ptr(),       \
                       (unsigned*)ticket.data_ptr(), cap / B - 1, (long)B,    \
                       x_row_bytes, y_row_bytes)
    switch (xu) {
        case 16: LAUNCH_BG(16); break;
        case 8: LAUNCH_BG(8); break;
        case 4: LAUNCH_BG(4); break;
        case 2: LAUNCH_BG(2); break;
        case 1: LAUNCH_BG(1); break;
        default: TORCH_CHECK(false, "batch_gather: unsupported element size");
    }
#undef LAUNCH_BG
    return {xb, yb};
}
