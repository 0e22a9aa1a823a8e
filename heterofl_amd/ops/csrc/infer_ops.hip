// Inference-side companions of the large-batch conv (conv_infer.hip):
//
// bn_relu_infer: eval-mode BatchNorm + ReLU with the running statistics
//   folded on the host into per-channel scale = w*rsqrt(var+eps) and
//   shift = b - mean*scale:  y = relu(x*scale[c] + shift[c]).  16-byte
//   vectorised when the plane size is a multiple of the vector width (every
//   vector then lies inside one channel plane); scalar otherwise.
//
// eval_metrics: every user's Local (label-split-masked) and the Global
//   (raw-logit) evaluation sums from one (N, C) logit matrix, replacing the
//   per-user host loop of the evaluation.  Users own CSR segments of sample
//   indices (a sample may belong to several users or to none).  Mask-then-CE
//   order as in the reference (src/models/resnet.py:152-157): logits of
//   classes outside the user's label split are set to 0, not -inf, before
//   softmax and argmax.  The prediction is the lowest index holding the
//   maximum.  Deterministic: pass 1 writes per-entry (loss, correct) terms,
//   pass 2 reduces each user's segment with one block in fixed order; no
//   float atomics.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f4;

__device__ __forceinline__ float bits2f(unsigned short v) {
    return __uint_as_float((unsigned)v << 16);
}
__device__ __forceinline__ unsigned short f2bits(float v) {
    __hip_bfloat16 b = __float2bfloat16(v);
    return *reinterpret_cast<unsigned short*>(&b);
}

__global__ void __launch_bounds__(256)
bn_relu_infer_vec_f32(const float* __restrict__ x,
                      const float* __restrict__ scale,
                      const float* __restrict__ shift, float* __restrict__ y,
                      long nvec, int C, int HW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvec) return;
    const int c = (int)((i * 4 / HW) % C);
    const float a = scale[c], b = shift[c];
    f4 v = *(const f4*)(x + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], a, b), 0.f);
    *(f4*)(y + i * 4) = v;
}

__global__ void __launch_bounds__(256)
bn_relu_infer_vec_bf16(const unsigned short* __restrict__ x,
                       const float* __restrict__ scale,
                       const float* __restrict__ shift,
                       unsigned short* __restrict__ y, long nvec, int C,
                       int HW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvec) return;
    const int c = (int)((i * 8 / HW) % C);
    const float a = scale[c], b = shift[c];
    u16x8 v = *(const u16x8*)(x + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        v[j] = f2bits(fmaxf(fmaf(bits2f(v[j]), a, b), 0.f));
    *(u16x8*)(y + i * 8) = v;
}

template <typename T>
__global__ void __launch_bounds__(256)
bn_relu_infer_scalar(const T* __restrict__ x, const float* __restrict__ scale,
                     const float* __restrict__ shift, T* __restrict__ y,
                     long total, int C, int HW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / HW) % C);
    st_f32(y + i, fmaxf(fmaf(ld_f32(x + i), scale[c], shift[c]), 0.f));
}

// pass 1: entries [0, nnz) are the users' CSR entries (masked terms),
// entries [nnz, nnz+N) are the samples themselves (raw-logit terms).
__global__ void __launch_bounds__(256)
eval_terms_kernel(const float* __restrict__ scores,
                  const long* __restrict__ labels,
                  const long* __restrict__ user_ptr,
                  const long* __restrict__ user_samples,
                  const float* __restrict__ label_mask,
                  float* __restrict__ terms, long nnz, long N, int U, int C) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz + N) return;
    long n;
    const float* mk = nullptr;
    if (e < nnz) {
        // owning user: last u with user_ptr[u] <= e (empty users skipped)
        int lo = 0, hi = U;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (user_ptr[mid] <= e) lo = mid; else hi = mid;
        }
        n = user_samples[e];
        mk = label_mask + (long)lo * C;
    } else {
        n = e - nnz;
    }
    if (n < 0 || n >= N) {  // malformed CSR entry: poison, never read
        terms[2 * e] = NAN;
        terms[2 * e + 1] = NAN;
        return;
    }
    const float* s = scores + n * C;
    const long yl = labels[n];
    if (yl < 0 || yl >= C) {
        terms[2 * e] = NAN;
        terms[2 * e + 1] = NAN;
        return;
    }
    float mx = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        float v = s[c];
        if (mk) v = mk[c] != 0.f ? v : 0.f;
        if (v > mx) { mx = v; arg = c; }  // strict: lowest index wins ties
    }
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
        float v = s[c];
        if (mk) v = mk[c] != 0.f ? v : 0.f;
        sum += expf(v - mx);
    }
    float vy = s[yl];
    if (mk) vy = mk[yl] != 0.f ? vy : 0.f;
    terms[2 * e] = mx + logf(sum) - vy;
    terms[2 * e + 1] = (arg == yl) ? 1.f : 0.f;
}

// pass 2: block u < U reduces user u's segment, block U the global terms.
// Thread t sums elements t, t+256, ... in order, then a fixed LDS tree.
__global__ void __launch_bounds__(256)
eval_reduce_kernel(const float* __restrict__ terms,
                   const long* __restrict__ user_ptr, float* __restrict__ out,
                   long nnz, long N, int U) {
    __shared__ float s_loss[256], s_corr[256];
    const int u = blockIdx.x;
    long b, e;
    if (u < U) {
        b = max(0L, user_ptr[u]);
        e = min(nnz, user_ptr[u + 1]);
    }
    else { b = nnz; e = nnz + N; }
    float loss = 0.f, corr = 0.f;
    for (long i = b + threadIdx.x; i < e; i += 256) {
        loss += terms[2 * i];
        corr += terms[2 * i + 1];
    }
    s_loss[threadIdx.x] = loss;
    s_corr[threadIdx.x] = corr;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            s_loss[threadIdx.x] += s_loss[threadIdx.x + off];
            s_corr[threadIdx.x] += s_corr[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[3 * u] = s_loss[0];
        out[3 * u + 1] = s_corr[0];
        out[3 * u + 2] = (float)(e - b);
    }
}

}  // namespace

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

at::Tensor bn_relu_infer(at::Tensor x, at::Tensor scale, at::Tensor shift) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2);
    TORCH_CHECK(scale.scalar_type() == at::kFloat
                && shift.scalar_type() == at::kFloat
                && scale.is_contiguous() && shift.is_contiguous());
    const long total = x.numel();
    const int C = x.size(1);
    TORCH_CHECK(scale.numel() == C && shift.numel() == C,
                "bn_relu_infer: scale/shift must have one entry per channel");
    auto y = at::empty_like(x);
    if (total == 0) return y;
    const int HW = (int)(total / ((long)x.size(0) * C));
    auto stream = at::hip::getCurrentHIPStream();
    const bool aligned = ((uintptr_t)x.data_ptr() % 16 == 0)
                         && ((uintptr_t)y.data_ptr() % 16 == 0);
    const float* sc = scale.data_ptr<float>();
    const float* sh = shift.data_ptr<float>();
    if (x.scalar_type() == at::kFloat) {
        if (aligned && HW % 4 == 0) {
            const long nvec = total / 4;
            hipLaunchKernelGGL(bn_relu_infer_vec_f32,
                               dim3((unsigned)((nvec + 255) / 256)), dim3(256),
                               0, stream, x.data_ptr<float>(), sc, sh,
                               y.data_ptr<float>(), nvec, C, HW);
        } else {
            hipLaunchKernelGGL(bn_relu_infer_scalar<float>,
                               dim3((unsigned)((total + 255) / 256)),
                               dim3(256), 0, stream, x.data_ptr<float>(), sc,
                               sh, y.data_ptr<float>(), total, C, HW);
        }
    } else if (x.scalar_type() == at::kBFloat16) {
        if (aligned && HW % 8 == 0) {
            const long nvec = total / 8;
            hipLaunchKernelGGL(bn_relu_infer_vec_bf16,
                               dim3((unsigned)((nvec + 255) / 256)), dim3(256),
                               0, stream, (const unsigned short*)x.data_ptr(),
                               sc, sh, (unsigned short*)y.data_ptr(), nvec, C,
                               HW);
        } else {
            hipLaunchKernelGGL(bn_relu_infer_scalar<__hip_bfloat16>,
                               dim3((unsigned)((total + 255) / 256)),
                               dim3(256), 0, stream,
                               (const __hip_bfloat16*)x.data_ptr(), sc, sh,
                               (__hip_bfloat16*)y.data_ptr(), total, C, HW);
        }
    } else {
        TORCH_CHECK(false, "bn_relu_infer: fp32 or bf16 only");
    }
    return y;
}

std::vector<at::Tensor> eval_metrics(at::Tensor scores, at::Tensor labels,
                                     at::Tensor user_ptr,
                                     at::Tensor user_samples,
                                     at::Tensor label_mask) {
    TORCH_CHECK(scores.is_cuda() && scores.is_contiguous()
                && scores.dim() == 2 && scores.scalar_type() == at::kFloat);
    const long N = scores.size(0);
    const int C = scores.size(1);
    const int U = (int)user_ptr.numel() - 1;
    const long nnz = user_samples.numel();
    TORCH_CHECK(U >= 0 && labels.numel() == N && (U > 0 || nnz == 0));
    TORCH_CHECK(labels.scalar_type() == at::kLong
                && user_ptr.scalar_type() == at::kLong
                && user_samples.scalar_type() == at::kLong
                && label_mask.scalar_type() == at::kFloat);
    TORCH_CHECK(labels.is_cuda() && user_ptr.is_cuda()
                && user_samples.is_cuda() && label_mask.is_cuda());
    TORCH_CHECK(labels.is_contiguous() && user_ptr.is_contiguous()
                && user_samples.is_contiguous()
                && label_mask.is_contiguous());
    TORCH_CHECK(label_mask.numel() == (long)U * C,
                "eval_metrics: label_mask must be (U, C)");
    auto opts = scores.options();
    auto terms = at::empty({nnz + N, 2}, opts);
    auto out = at::empty({(long)U + 1, 3}, opts);
    auto stream = at::hip::getCurrentHIPStream();
    if (nnz + N > 0)
        hipLaunchKernelGGL(eval_terms_kernel,
                           dim3((unsigned)((nnz + N + 255) / 256)), dim3(256),
                           0, stream, scores.data_ptr<float>(),
                           labels.data_ptr<long>(), user_ptr.data_ptr<long>(),
                           user_samples.data_ptr<long>(),
                           label_mask.data_ptr<float>(),
                           terms.data_ptr<float>(), nnz, N, U, C);
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(U + 1), dim3(256), 0, stream,
                       terms.data_ptr<float>(), user_ptr.data_ptr<long>(),
                       out.data_ptr<float>(), nnz, N, U);
    return {out.narrow(0, 0, U), out.select(0, U)};
}
