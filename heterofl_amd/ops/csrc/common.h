// Shared helpers for the gfx950 HIP kernels (CDNA4: wave64, 4xSIMD-32 CUs).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdlib>

#define WAVE 64

// MFMA operand / accumulator vectors and the 16-byte bf16 load
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// fp32 accumulate load for fp32 / bf16 tensors
template <typename T>
__device__ __forceinline__ float ld_f32(const T* p) { return (float)*p; }
template <>
__device__ __forceinline__ float ld_f32<__hip_bfloat16>(const __hip_bfloat16* p) {
    return __bfloat162float(*p);
}

template <typename T>
__device__ __forceinline__ void st_f32(T* p, float v) { *p = (T)v; }
template <>
__device__ __forceinline__ void st_f32<__hip_bfloat16>(__hip_bfloat16* p, float v) {
    *p = __float2bfloat16(v);
}

// 16 bytes of T (4 fp32 / 8 bf16) as raw bits <-> fp32 values, for kernels
// that move memory with dwordx4 accesses.  Both directions give the bits of
// ld_f32 / st_f32 on the single elements.
template <typename T>
__device__ __forceinline__ void unpack16(const uint4& r, float* f) {
    f[0] = __uint_as_float(r.x);
    f[1] = __uint_as_float(r.y);
    f[2] = __uint_as_float(r.z);
    f[3] = __uint_as_float(r.w);
}
template <>
__device__ __forceinline__ void unpack16<__hip_bfloat16>(const uint4& r,
                                                         float* f) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    return (unsigned)__bfloat16_as_ushort(__float2bfloat16(lo))
           | ((unsigned)__bfloat16_as_ushort(__float2bfloat16(hi)) << 16);
}
template <typename T>
__device__ __forceinline__ uint4 pack16(const float* f) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                      __float_as_uint(f[2]), __float_as_uint(f[3]));
}
template <>
__device__ __forceinline__ uint4 pack16<__hip_bfloat16>(const float* f) {
    return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]),
                      pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}

// A generic pointer known to point to global memory (one read from a table,
// say).  Loads through it are global_load, counted by vmcnt alone, so a batch
// of them stays in flight; through the generic pointer they are flat_load,
// and every batch is waited out to zero.
template <typename T>
using gptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ gptr<T> as_global(T* p) { return (gptr<T>)p; }
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// HETEROFL_STREAM_VEC=0 (read on every call, so one process can flip it)
// routes the BN+ReLU, split-reduce and clip+SGD launchers back to their
// one-element-per-lane kernels.
static inline bool stream_vec_on() {
    const char* e = std::getenv("HETEROFL_STREAM_VEC");
    return !(e && e[0] == '0');
}
static inline bool ptr_aligned(const void* p, unsigned long bytes) {
    return (reinterpret_cast<unsigned long>(p) & (bytes - 1)) == 0;
}

// block-wide sum of two values over blockDim.x threads (<=1024), LDS based.
// Returns (s1, s2) to every thread.  `scratch` must hold 2*blockDim.x/WAVE floats.
__device__ __forceinline__ void block_reduce2(float& v1, float& v2, float* scratch) {
    // wave reduce first
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        v1 += __shfl_down(v1, off, WAVE);
        v2 += __shfl_down(v2, off, WAVE);
    }
    const int wid = threadIdx.x / WAVE;
    const int nw = blockDim.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        scratch[2 * wid] = v1;
        scratch[2 * wid + 1] = v2;
    }
    __syncthreads();
    if (threadIdx.x < WAVE) {
        float a = (threadIdx.x < nw) ? scratch[2 * threadIdx.x] : 0.f;
        float b = (threadIdx.x < nw) ? scratch[2 * threadIdx.x + 1] : 0.f;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            a += __shfl_down(a, off, WAVE);
            b += __shfl_down(b, off, WAVE);
        }
        if (threadIdx.x == 0) { scratch[0] = a; scratch[1] = b; }
    }
    __syncthreads();
    v1 = scratch[0];
    v2 = scratch[1];
    __syncthreads();
}
