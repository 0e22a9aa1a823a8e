// Hand-written gfx950 MFMA implicit-GEMM grouped convolution (K1/K2 of
// SURVEY.md §2b): forward (+fused residual add), backward-data and
// deterministic split-P backward-weight for the NCHW 3x3/1x1 convs of
// HeteroFL's batched client models (reference conv sites:
// src/models/resnet.py:33-42, src/models/conv.py:29).
//
// Why hand-written: the round's convs are tiny (batch 10, 32x32 .. 4x4
// spatial, grouped over R clients) — MIOpen/CK fall back to naive or
// heavyweight xdl kernels at 50-225us per call plus im2col/transpose glue
// (profiles/kstats_r01_fused_v1.txt).  One direct implicit-GEMM kernel per
// direction, bf16 inputs with fp32 MFMA accumulate (or exact-f32 MFMA for
// the fp32 path), no im2col materialization, fp32 weight gradients.
//
// GEMM view (per group g):
//   fwd:  y[m,p]  = sum_k  w[m,k] * patch[k,p]      M=Cout, K=Cin*kh*kw,
//                                                   P=N*OH*OW
//   bwdW: dw[m,k] = sum_p  dy[m,p] * patch[k,p]     (split-P partials +
//                                                    deterministic reduce)
//   bwdD: dx[c,q] = sum_j  w'[c,j] * dyp[j,q]       j=Cout*kh*kw, q=N*H*W
//
// Tiling: 256-thread workgroups (4 waves), 64x64 output tile, BK=32,
// mfma_f32_16x16x32_bf16 (or 8x mfma_f32_16x16x4_f32), LDS tiles stored
// [row][k] with +8-element padding; per-block index-decomposition tables
// (pixel -> (n, ihbase, iwbase)) remove the per-element div/mod chains from
// the gather loaders.  Fragment layout (verified on hardware by
// tests/test_gpu.py::test_mfma_probe_layout): A: lane l holds
// A[row=l%16][k=(l/16)*8+j]; B: B[k=(l/16)*8+j][col=l%16]; C/D:
// row=(l/16)*4+reg, col=l%16.
//
// Kernel families, fastest route first (host layer at the bottom routes):
//   resident  conv_{fwd,bwd_data,bwd_weight}_resident_kernel: window staged
//             once per block (per sample segment for bwd-weight) as raw T,
//             offset tables instead of k-loop div/mod, double-buffered
//             tiles, one barrier per k-step.  Taken wherever the staged
//             geometry holds and the slice fits 64 KB of LDS;
//             HETEROFL_CONV_RESIDENT=0 turns it off.
//   staged    conv_*_staged_kernel: window restaged per k-step; the
//             fallback and the bit-exact oracle of the resident kernels.
//   tabled    conv_fwd_tabled_kernel, conv_bwd_data{,_s2}_tabled_kernel,
//             conv_bwd_weight_tabled_kernel: any geometry; the reduction
//             index decode and the bounds tests come from per-block tables
//             and per-pixel tap masks built in the prologue, tiles are
//             double-buffered.  Taken on the gather routes for bf16/fp32
//             while the slice's table fits its capacity;
//             HETEROFL_CONV_TABLED=0 turns it off.
//   gather    conv_fwd_kernel, conv_bwd_data{,_s2}_kernel,
//             conv_bwd_weight_kernel: any geometry, fp8 instantiations; the
//             fallback and the bit-exact oracle of the tabled kernels.
// The multi-sample staged fwd / bwd-data kernels and the opt-in switch that
// selected them measured slower than the gather kernels (profiles/NOTES.md)
// and were removed; commit 67e6a3a is the last that carries them.
#include "common.h"

constexpr int BM = 64;
constexpr int BP = 64;
constexpr int BK = 32;
constexpr int LDK = BK + 8;  // padded k-stride for [.][k]-contiguous tiles

// one 16x16 MFMA accumulation over a BK=32 K-slab, element type T
template <typename T>
__device__ __forceinline__ f32x4 mfma_tile(const T* a_row, const T* b_col,
                                           f32x4 acc);

template <>
__device__ __forceinline__ f32x4 mfma_tile<__hip_bfloat16>(
        const __hip_bfloat16* a_row, const __hip_bfloat16* b_col, f32x4 acc) {
    const int l = threadIdx.x & (WAVE - 1);
    const int kb = (l >> 4) * 8;
    bf16x8 a = *(const bf16x8*)(a_row + kb);
    bf16x8 b = *(const bf16x8*)(b_col + kb);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}

template <>
__device__ __forceinline__ f32x4 mfma_tile<float>(const float* a_row,
                                                  const float* b_col,
                                                  f32x4 acc) {
    const int l = threadIdx.x & (WAVE - 1);
    const int ko = l >> 4;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[q * 4 + ko],
                                                   b_col[q * 4 + ko], acc, 0,
                                                   0, 0);
    }
    return acc;
}


// store 8 fp32 values as one contiguous 16B (bf16) / 32B (f32) LDS write
__device__ __forceinline__ void st8_lds(__hip_bfloat16* dst, const float* v) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (__bf16)v[j];
    *(bf16x8*)dst = t;
}
__device__ __forceinline__ void st8_lds(float* dst, const float* v) {
    typedef __attribute__((ext_vector_type(4))) float f4;
    *(f4*)dst = *(const f4*)v;
    *(f4*)(dst + 4) = *(const f4*)(v + 4);
}

// fp8 LDS tile element tags (OCP formats; gfx950 fp8 MFMA is e4m3/e5m2 —
// cdna_hip_programming.md §4).  e4m3 carries weights/activations, e5m2
// gradients; the mixed mfma_f32_16x16x32_{fp8,bf8}_{fp8,bf8} forms multiply
// them directly (CDNA4 fp8 MFMA, BASELINE config 5).
#include <hip/hip_fp8.h>
struct e4m3 { unsigned char x; };
struct e5m2 { unsigned char x; };
typedef long long i64;

__device__ __forceinline__ void st8_lds(e4m3* dst, const float* v) {
    unsigned char t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        t[j] = __hip_cvt_float_to_fp8(v[j], __HIP_SATFINITE, __HIP_E4M3);
    *(i64*)dst = *(const i64*)t;
}
__device__ __forceinline__ void st8_lds(e5m2* dst, const float* v) {
    unsigned char t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        t[j] = __hip_cvt_float_to_fp8(v[j], __HIP_SATFINITE, __HIP_E5M2);
    *(i64*)dst = *(const i64*)t;
}

// mixed-type MFMA: a_row/b_col point at the lane's LDS rows; the k-offset
// (l/16)*8 selects the lane's 8-element fragment (layout as above).
template <typename TA, typename TB>
__device__ __forceinline__ f32x4 mfma_tile2(const TA* a_row, const TB* b_col,
                                            f32x4 acc) {
    return mfma_tile<TA>(a_row, b_col, acc);  // TA == TB fast path
}
template <>
__device__ __forceinline__ f32x4 mfma_tile2<e4m3, e4m3>(const e4m3* a_row,
                                                        const e4m3* b_col,
                                                        f32x4 acc) {
    const int l = threadIdx.x & (WAVE - 1);
    const int kb = (l >> 4) * 8;
    i64 a = *(const i64*)(a_row + kb);
    i64 b = *(const i64*)(b_col + kb);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma_tile2<e4m3, e5m2>(const e4m3* a_row,
                                                        const e5m2* b_col,
                                                        f32x4 acc) {
    const int l = threadIdx.x & (WAVE - 1);
    const int kb = (l >> 4) * 8;
    i64 a = *(const i64*)(a_row + kb);
    i64 b = *(const i64*)(b_col + kb);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(a, b, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma_tile2<e5m2, e4m3>(const e5m2* a_row,
                                                        const e4m3* b_col,
                                                        f32x4 acc) {
    const int l = threadIdx.x & (WAVE - 1);
    const int kb = (l >> 4) * 8;
    i64 a = *(const i64*)(a_row + kb);
    i64 b = *(const i64*)(b_col + kb);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(a, b, acc, 0, 0, 0);
}

struct ConvGeom {
    int G;
    int N, H, W;
    int Cin, Cout;
    int OH, OW;
    int khw;
    int stride, pad;
};

// Where a block and its threads sit, the same in every conv kernel (two
// spell it out, see there): blockIdx.z = split * G + group; blockIdx.x/y =
// the 64x64 output tile (row0 = x * BM, col0 = y * BP); each wave owns the
// 32x32 quadrant (wm, wp) of it.
struct TileCoord { int g, sp, row0, col0, tid, l, wm, wp; };
__device__ __forceinline__ TileCoord tile_coord(int G) {
    TileCoord t;
    t.g = blockIdx.z % G;
    t.sp = blockIdx.z / G;
    t.row0 = blockIdx.x * BM;
    t.col0 = blockIdx.y * BP;
    t.tid = threadIdx.x;
    t.l = t.tid & (WAVE - 1);
    const int wave = t.tid / WAVE;
    t.wm = (wave >> 1) * 32;
    t.wp = (wave & 1) * 32;
    return t;
}

// One accumulator element of the fwd epilogue: bias + residual and the cast
// store when unsplit, else the split's fp32 partial slab (conv_out_reduce
// applies bias/residual).  ch = g*Cout + m, off = the element's y offset.
template <typename T>
__device__ __forceinline__ void fwd_store(float v, long off, int ch,
                                          const float* __restrict__ bias,
                                          const T* __restrict__ residual,
                                          T* __restrict__ y,
                                          float* __restrict__ partial,
                                          long slab, int splitk) {
    if (splitk == 1) {
        if (bias) v += bias[ch];
        if (residual) v += ld_f32(residual + off);
        st_f32(y + off, v);
    } else {
        partial[slab + off] = v;
    }
}


// -------------------------------------------------------------- fwd kernel
// grid: (ceil(M/BM), ceil(P/BP), G).  Optional residual is added in the
// epilogue (the ResNet block's `out += shortcut`, src/models/resnet.py:49).
// splitk > 1: each split writes fp32 partial slabs (sp, N*G*Cout*OHW);
// conv_out_reduce_kernel sums them in fixed order and applies bias/residual.
template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                const float* __restrict__ bias, const T* __restrict__ residual,
                T* __restrict__ y, float* __restrict__ partial, ConvGeom gm,
                int splitk) {
    __shared__ TA a_lds[2][BM][LDK];
    __shared__ TB b_lds[2][BP][LDK];
    __shared__ int t_ihb[BP], t_iwb[BP];
    __shared__ long t_xbase[BP], t_ybase[BP];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, p0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int nkc = ((K + BK - 1) / BK + splitk - 1) / splitk;  // BK-chunks
    const int ks = sp * nkc * BK;
    const int ke = min(K, ks + nkc * BK);

    // per-block pixel decomposition tables
    if (tid < BP) {
        const int p = p0 + tid;
        if (p < P) {
            const int n = p / OHW, hw = p - n * OHW;
            const int oh = hw / gm.OW, ow = hw - oh * gm.OW;
            t_ihb[tid] = oh * gm.stride - gm.pad;
            t_iwb[tid] = ow * gm.stride - gm.pad;
            t_xbase[tid] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW;
            t_ybase[tid] = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW
                           + hw;
        } else {
            t_ihb[tid] = 1 << 28;  // forces out-of-bounds -> zeros
            t_iwb[tid] = 1 << 28;
            t_xbase[tid] = 0;
            t_ybase[tid] = -1;
        }
    }
    __syncthreads();

    f32x4 acc[2][2] = {};
    const int mm_a = tid >> 2, kkb = (tid & 3) * 8;
    const int pp_b = tid >> 2;
    float va[8], vb[8];
    // loader for one K-step into registers (2-phase: issue next tile's
    // loads before this tile's MFMA so HBM/L2 latency hides under it)
    auto load_regs = [&](int k0) {
        const int m = m0 + mm_a;
        const float* wrow = w + (long)(g * gm.Cout + m) * K + k0 + kkb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + kkb + j;
            va[j] = (m < M && k < K) ? wrow[j] : 0.f;
        }
        // incremental k -> (cin, kh, kw): one divide per 8 contiguous k
        // (runtime integer divides cost ~60 VALU cycles each)
        int k = k0 + kkb;
        int cin = k / kk2, r = k - cin * kk2;
        int kh = r / gm.khw, kw = r - kh * gm.khw;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vb[j] = 0.f;
            if (k + j < K) {
                const int ih = t_ihb[pp_b] + kh, iw = t_iwb[pp_b] + kw;
                if (ih >= 0 && ih < gm.H && iw >= 0 && iw < gm.W)
                    vb[j] = ld_f32(x + t_xbase[pp_b] + (long)cin * HW
                                   + ih * gm.W + iw);
            }
            if (++kw == gm.khw) {
                kw = 0;
                if (++kh == gm.khw) {
                    kh = 0;
                    ++cin;
                }
            }
        }
    };
    // double-buffered k-loop: ONE barrier per iteration; tile t+1's loads
    // stay in flight across tile t's whole MFMA phase
    load_regs(ks);
    st8_lds(&a_lds[0][mm_a][kkb], va);
    st8_lds(&b_lds[0][pp_b][kkb], vb);
    if (ks + BK < ke) load_regs(ks + BK);
    __syncthreads();
    int cur = 0;
    for (int k0 = ks; k0 < ke; k0 += BK) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (k0 + BK < ke) {
            st8_lds(&a_lds[cur ^ 1][mm_a][kkb], va);
            st8_lds(&b_lds[cur ^ 1][pp_b][kkb], vb);
            if (k0 + 2 * BK < ke) load_regs(k0 + 2 * BK);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cout * OHW;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int pp = wp + fp * 16 + (l & 15);
            const long yb = t_ybase[pp];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (m < M && yb >= 0)
                    fwd_store(acc[fm][fp][r], yb + (long)m * OHW,
                              g * gm.Cout + m, bias, residual, y, partial,
                              slab, splitk);
            }
        }
}

// sum split-K partials in fixed order; add bias/residual; cast to T
template <typename T>
__global__ void __launch_bounds__(256)
conv_out_reduce_kernel(const float* __restrict__ partial,
                       const float* __restrict__ bias,
                       const T* __restrict__ residual, T* __restrict__ out,
                       long total, long chanstride, int nchan, int splitk) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float v = 0.f;
    for (int sp = 0; sp < splitk; ++sp) v += partial[(long)sp * total + i];
    if (bias) v += bias[(i / chanstride) % nchan];
    if (residual) v += ld_f32(residual + i);
    st_f32(out + i, v);
}

// Four consecutive outputs per lane of a split reduce: the slabs' float4 at
// vector index i4, RED_U loads issued before the first add, each output still
// adding its partials in sp = 0, 1, ... order from 0.f (the bits of the
// one-float-per-lane kernels, which HETEROFL_STREAM_VEC=0 runs).
constexpr int RED_U = 8;

__device__ __forceinline__ float4 sum_slabs_f4(const float4* __restrict__ p,
                                               long stride4, int split) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int sp = 0;
    for (; sp + RED_U <= split; sp += RED_U) {
        float4 a[RED_U];
#pragma unroll
        for (int u = 0; u < RED_U; ++u) a[u] = p[(sp + u) * stride4];
#pragma unroll
        for (int u = 0; u < RED_U; ++u) {
            s.x += a[u].x;
            s.y += a[u].y;
            s.z += a[u].z;
            s.w += a[u].w;
        }
    }
    if (sp + 4 <= split) {
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = p[(sp + u) * stride4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s.x += a[u].x;
            s.y += a[u].y;
            s.z += a[u].z;
            s.w += a[u].w;
        }
        sp += 4;
    }
    if (sp + 2 <= split) {
        const float4 a0 = p[sp * stride4], a1 = p[(sp + 1) * stride4];
        s.x += a0.x; s.y += a0.y; s.z += a0.z; s.w += a0.w;
        s.x += a1.x; s.y += a1.y; s.z += a1.z; s.w += a1.w;
        sp += 2;
    }
    if (sp < split) {
        const float4 a0 = p[sp * stride4];
        s.x += a0.x; s.y += a0.y; s.z += a0.z; s.w += a0.w;
    }
    return s;
}

// BIAS: 0 none (every bwd-data call, bias-free fwd): no channel arithmetic;
// 1: chanstride % 4 == 0, one channel per vector; 2: a vector may straddle
// channels, one index per element.  IDX is int when total < 2^31.
// Needs total % 4 == 0, 16-byte aligned partial, 4-element aligned
// residual / out.
template <typename T, int BIAS, typename IDX>
__global__ void __launch_bounds__(256)
conv_out_reduce_vec_kernel(const float* __restrict__ partial,
                           const float* __restrict__ bias,
                           const T* __restrict__ residual,
                           T* __restrict__ out, long total, long chanstride,
                           int nchan, int splitk) {
    const long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total4 = total >> 2;
    if (i4 >= total4) return;
    const float4 s = sum_slabs_f4((const float4*)partial + i4, total4, splitk);
    float v[4] = {s.x, s.y, s.z, s.w};
    if (BIAS == 1) {
        const float bv =
            bias[((IDX)(i4 * 4) / (IDX)chanstride) % (IDX)nchan];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bv;
    } else if (BIAS == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] += bias[((IDX)(i4 * 4 + e) / (IDX)chanstride) % (IDX)nchan];
    }
    if (sizeof(T) == 4) {
        if (residual) {
            const float4 r = ((const float4*)residual)[i4];
            v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
        }
        ((float4*)out)[i4] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        if (residual) {
            const uint2 r = ((const uint2*)residual)[i4];
            v[0] += __uint_as_float(r.x << 16);
            v[1] += __uint_as_float(r.x & 0xffff0000u);
            v[2] += __uint_as_float(r.y << 16);
            v[3] += __uint_as_float(r.y & 0xffff0000u);
        }
        ((uint2*)out)[i4] = make_uint2(pack_bf16x2(v[0], v[1]),
                                       pack_bf16x2(v[2], v[3]));
    }
}

// -------------------------------------------------------- bwd-data kernel
template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_bwd_data_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                     T* __restrict__ dx, float* __restrict__ partial,
                     ConvGeom gm, int splitk) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ int t_oh[BP], t_ow[BP];  // ih+pad, iw+pad (pre-division)
    __shared__ long t_dybase[BP], t_xbase[BP];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int c0 = tc.row0, q0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int J = gm.Cout * kk2;
    const int K = gm.Cin * kk2;
    const int HW = gm.H * gm.W;
    const int Q = gm.N * HW;
    const int OHW = gm.OH * gm.OW;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;

    if (tid < BP) {
        const int q = q0 + tid;
        if (q < Q) {
            const int n = q / HW, hw = q - n * HW;
            const int ih = hw / gm.W, iw = hw - ih * gm.W;
            t_oh[tid] = ih + gm.pad;
            t_ow[tid] = iw + gm.pad;
            t_dybase[tid] = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout)
                            * OHW;
            t_xbase[tid] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW
                           + hw;
        } else {
            t_oh[tid] = -(1 << 28);
            t_ow[tid] = -(1 << 28);
            t_dybase[tid] = 0;
            t_xbase[tid] = -1;
        }
    }
    __syncthreads();

    const int njc = ((J + BK - 1) / BK + splitk - 1) / splitk;
    const int js = sp * njc * BK;
    const int je = min(J, js + njc * BK);
    f32x4 acc[2][2] = {};
    const int cc_a = tid >> 2, jjb = (tid & 3) * 8;
    float va[8], vb[8];
    auto load_regs = [&](int j0) {
        const int c = c0 + cc_a;
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int j = j0 + jjb + j8;
            va[j8] = 0.f;
            if (c < gm.Cin && j < J) {
                const int cout = j / kk2, r = j - cout * kk2;
                va[j8] = w[(long)(g * gm.Cout + cout) * K + c * kk2 + r];
            }
        }
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int j = j0 + jjb + j8;
            vb[j8] = 0.f;
            if (j < J) {
                const int cout = j / kk2, r = j - cout * kk2;
                const int kh = r / gm.khw, kw = r - kh * gm.khw;
                const int ohs = t_oh[cc_a] - kh, ows = t_ow[cc_a] - kw;
                if (ohs >= 0 && ows >= 0) {
                    if (gm.stride == 1) {
                        if (ohs < gm.OH && ows < gm.OW)
                            vb[j8] = ld_f32(dy + t_dybase[cc_a]
                                            + (long)cout * OHW
                                            + ohs * gm.OW + ows);
                    } else if ((ohs & 1) == 0 && (ows & 1) == 0) {
                        const int oh = ohs >> 1, ow = ows >> 1;
                        if (oh < gm.OH && ow < gm.OW)
                            vb[j8] = ld_f32(dy + t_dybase[cc_a]
                                            + (long)cout * OHW
                                            + oh * gm.OW + ow);
                    }
                }
            }
        }
    };
    if (js < je) load_regs(js);
    for (int j0 = js; j0 < je; j0 += BK) {
        st8_lds(&a_lds[cc_a][jjb], va);
        st8_lds(&b_lds[cc_a][jjb], vb);
        __syncthreads();
        if (j0 + BK < je) load_regs(j0 + BK);
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        __syncthreads();
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cin * HW;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int qq = wp + fp * 16 + (l & 15);
            const long xb = t_xbase[qq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (c < gm.Cin && xb >= 0) {
                    if (splitk == 1)
                        st_f32(dx + xb + (long)c * HW, acc[fm][fp][r]);
                    else
                        partial[slab + xb + (long)c * HW] = acc[fm][fp][r];
                }
            }
        }
}


// ------------------------------------------- stride-2 bwd-data (parity)
// For stride 2 only 1/4 of the (kh, kw) taps can contribute to a given
// input pixel (ohs/ows parity).  Pixels are tiled by parity class
// (ph, pw): each class is a dense (H/2, W/2) sub-image with a compressed
// tap list, so no MFMA work is spent on dead taps.  grid.y = 4 * tiles.
template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_bwd_data_s2_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                        T* __restrict__ dx, float* __restrict__ partial,
                        ConvGeom gm, int splitk, int nyp) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ int t_oh2[BP], t_ow2[BP];
    __shared__ long t_dybase[BP], t_xbase[BP];
    // (tile_coord() spelled out: blockIdx.y also carries the parity class,
    // and going through it reorders this kernel's instructions)
    const int g = blockIdx.z % gm.G;
    const int sp = blockIdx.z / gm.G;
    const int c0 = blockIdx.x * BM;
    const int cls = blockIdx.y / nyp;
    const int q0 = (blockIdx.y - cls * nyp) * BP;
    const int ph = cls >> 1, pw = cls & 1;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int H2 = gm.H >> 1, W2 = gm.W >> 1;
    const int HW2 = H2 * W2;
    const int Qp = gm.N * HW2;
    const int HW = gm.H * gm.W;
    const int OHW = gm.OH * gm.OW;
    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int wm = (wave >> 1) * 32;
    const int wp = (wave & 1) * 32;
    // compressed tap lists for this parity class (khw <= 3)
    int lkh[3], lkw[3], skh[3], skw[3];
    int nkh = 0, nkw = 0;
    for (int kh = 0; kh < gm.khw; ++kh)
        if (((ph + gm.pad - kh) & 1) == 0) {
            lkh[nkh] = kh;
            skh[nkh] = (ph + gm.pad - kh) >> 1;
            ++nkh;
        }
    for (int kw = 0; kw < gm.khw; ++kw)
        if (((pw + gm.pad - kw) & 1) == 0) {
            lkw[nkw] = kw;
            skw[nkw] = (pw + gm.pad - kw) >> 1;
            ++nkw;
        }
    const int tap2 = nkh * nkw;
    const int J = gm.Cout * tap2;

    if (tid < BP) {
        const int q = q0 + tid;
        if (q < Qp) {
            const int n = q / HW2, hw2 = q - n * HW2;
            const int ih2 = hw2 / W2, iw2 = hw2 - ih2 * W2;
            t_oh2[tid] = ih2;
            t_ow2[tid] = iw2;
            t_dybase[tid] = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout)
                            * OHW;
            t_xbase[tid] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW
                           + (2 * ih2 + ph) * gm.W + (2 * iw2 + pw);
        } else {
            t_oh2[tid] = -(1 << 28);
            t_ow2[tid] = -(1 << 28);
            t_dybase[tid] = 0;
            t_xbase[tid] = -1;
        }
    }
    __syncthreads();

    const int njc = ((J + BK - 1) / BK + splitk - 1) / splitk;
    const int js = sp * njc * BK;
    const int je = min(J, js + njc * BK);
    f32x4 acc[2][2] = {};
    const int cc_a = tid >> 2, jjb = (tid & 3) * 8;
    float va[8], vb[8];
    auto load_regs = [&](int j0) {
        const int c = c0 + cc_a;
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int j = j0 + jjb + j8;
            va[j8] = 0.f;
            if (c < gm.Cin && j < J) {
                const int cout = j / tap2, rr = j - cout * tap2;
                const int kh = lkh[rr / nkw], kw = lkw[rr - (rr / nkw) * nkw];
                va[j8] = w[(long)(g * gm.Cout + cout) * K + c * kk2
                           + kh * gm.khw + kw];
            }
        }
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int j = j0 + jjb + j8;
            vb[j8] = 0.f;
            if (j < J) {
                const int cout = j / tap2, rr = j - cout * tap2;
                const int a = rr / nkw, b = rr - a * nkw;
                const int oh = t_oh2[cc_a] + skh[a];
                const int ow = t_ow2[cc_a] + skw[b];
                if (oh >= 0 && oh < gm.OH && ow >= 0 && ow < gm.OW)
                    vb[j8] = ld_f32(dy + t_dybase[cc_a] + (long)cout * OHW
                                    + oh * gm.OW + ow);
            }
        }
    };
    if (js < je) load_regs(js);
    for (int j0 = js; j0 < je; j0 += BK) {
        st8_lds(&a_lds[cc_a][jjb], va);
        st8_lds(&b_lds[cc_a][jjb], vb);
        __syncthreads();
        if (j0 + BK < je) load_regs(j0 + BK);
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        __syncthreads();
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cin * HW;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int qq = wp + fp * 16 + (l & 15);
            const long xb = t_xbase[qq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (c < gm.Cin && xb >= 0) {
                    if (splitk == 1)
                        st_f32(dx + xb + (long)c * HW, acc[fm][fp][r]);
                    else
                        partial[slab + xb + (long)c * HW] = acc[fm][fp][r];
                }
            }
        }
}

// ------------------------------------------------------ bwd-weight kernel
// Writes per-split partials (splitp, G*Cout*K) when splitp > 1; a
// deterministic reduce kernel sums them in fixed order (no atomics, so the
// hipGraph-captured step replays bit-identically run to run).
template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_bwd_weight_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                       float* __restrict__ out, ConvGeom gm, int splitp) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ int t_kcin[BP], t_kkh[BP], t_kkw[BP];   // per-block k tables
    __shared__ int t_ihb[BK], t_iwb[BK];               // per-step p tables
    __shared__ long t_xb[BK], t_dyb[BK];
    // (tile_coord() spelled out: going through it reorders this kernel's
    // prologue instructions, and the kernels are held instruction-identical)
    const int g = blockIdx.z % gm.G;
    const int sp = blockIdx.z / gm.G;
    const int m0 = blockIdx.x * BM;
    const int k0 = blockIdx.y * BP;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const long GK = (long)gm.G * gm.Cout * K;  // one split's slab
    const int pchunk = (P + splitp - 1) / splitp;
    const int pstart = sp * pchunk;
    const int pend = min(P, pstart + pchunk);
    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int wm = (wave >> 1) * 32;
    const int wp = (wave & 1) * 32;
    f32x4 acc[2][2] = {};

    if (tid < BP) {
        const int k = k0 + tid;
        if (k < K) {
            const int cin = k / kk2, r = k - cin * kk2;
            t_kcin[tid] = cin;
            t_kkh[tid] = r / gm.khw;
            t_kkw[tid] = r - (r / gm.khw) * gm.khw;
        } else {
            t_kcin[tid] = 0;
            t_kkh[tid] = 1 << 28;
            t_kkw[tid] = 1 << 28;
        }
    }

    for (int p0 = pstart; p0 < pend; p0 += BK) {
        __syncthreads();
        if (tid < BK) {
            const int p = p0 + tid;
            if (p < pend) {
                const int n = p / OHW, hw = p - n * OHW;
                const int oh = hw / gm.OW, ow = hw - oh * gm.OW;
                t_ihb[tid] = oh * gm.stride - gm.pad;
                t_iwb[tid] = ow * gm.stride - gm.pad;
                t_xb[tid] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW;
                t_dyb[tid] = ((long)n * gm.G * gm.Cout
                              + (long)g * gm.Cout) * OHW + hw;
            } else {
                t_ihb[tid] = 1 << 28;
                t_iwb[tid] = 1 << 28;
                t_xb[tid] = 0;
                t_dyb[tid] = -1;
            }
        }
        __syncthreads();
        {   // a tile rows: 64 rows x 32 p; thread owns 8 contiguous p
            const int mm = (tid >> 2) & 63, ppb = (tid & 3) * 8;
            const int m = m0 + mm;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pp = ppb + j;
                v[j] = (m < M && t_dyb[pp] >= 0)
                           ? ld_f32(dy + t_dyb[pp] + (long)m * OHW) : 0.f;
            }
            st8_lds(&a_lds[mm][ppb], v);
        }
        {
            const int kk = (tid >> 2) & 63, ppb = (tid & 3) * 8;
            const int k = k0 + kk;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pp = ppb + j;
                v[j] = 0.f;
                if (k < K) {
                    const int ih = t_ihb[pp] + t_kkh[kk];
                    const int iw = t_iwb[pp] + t_kkw[kk];
                    if (ih >= 0 && ih < gm.H && iw >= 0 && iw < gm.W)
                        v[j] = ld_f32(x + t_xb[pp] + (long)t_kcin[kk] * HW
                                      + ih * gm.W + iw);
                }
            }
            st8_lds(&b_lds[kk][ppb], v);
        }
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        __syncthreads();
    }
    float* slab = out + (long)sp * GK;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                const int k = k0 + wp + fp * 16 + (l & 15);
                if (m < M && k < K)
                    slab[(long)(g * gm.Cout + m) * K + k] = acc[fm][fp][r];
            }
}

__global__ void __launch_bounds__(256)
splitp_reduce_kernel(const float* __restrict__ partials,
                     float* __restrict__ dw, long GK, int splitp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= GK) return;
    float s = 0.f;
    for (int sp = 0; sp < splitp; ++sp) s += partials[(long)sp * GK + i];
    dw[i] = s;
}

// GK % 4 == 0 and 16-byte aligned bases: four outputs per lane
__global__ void __launch_bounds__(256)
splitp_reduce_vec_kernel(const float* __restrict__ partials,
                         float* __restrict__ dw, long GK, int splitp) {
    const long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long GK4 = GK >> 2;
    if (i4 >= GK4) return;
    ((float4*)dw)[i4] = sum_slabs_f4((const float4*)partials + i4, GK4,
                                     splitp);
}


// ---------------------------------------------- staged fwd (im2col in LDS)
// When a BP-pixel tile lies inside one sample and spans whole output rows
// (OHW %% BP == 0 and BP %% OW == 0), the tile's input window is a dense
// (channels x rows x width) slab: stage it into LDS with coalesced loads
// once per k-step and build the implicit-GEMM B tile from LDS.  This
// replaces 16 scattered 2-byte global loads per thread per k-step (the
// measured bound: 65%% wave-wait, profiles/pmc_conv_fwd_r01.txt) with ~90
// coalesced transactions per block.
constexpr int WIN_CH = BK / 9 + 2;   // channels a BK k-slab can touch (3x3)
constexpr int WIN_ROWS = 16;         // (BP/OW - 1)*stride + khw  (<= 16)
constexpr int WIN_W = 40;            // padded input width (W + 2*pad <= 34)

template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_fwd_staged_kernel(const T* __restrict__ x, const float* __restrict__ w,
                       const float* __restrict__ bias,
                       const T* __restrict__ residual, T* __restrict__ y,
                       float* __restrict__ partial, ConvGeom gm, int splitk) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ float win[WIN_CH][WIN_ROWS][WIN_W];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, p0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int nkc = ((K + BK - 1) / BK + splitk - 1) / splitk;
    const int ks = sp * nkc * BK;
    const int ke = min(K, ks + nkc * BK);
    // tile geometry: one sample, whole output rows
    const int n = p0 / OHW;
    const int oh0 = (p0 - n * OHW) / gm.OW;
    const int nrow_out = BP / gm.OW;
    const int rows_in = (nrow_out - 1) * gm.stride + gm.khw;
    const int ih0 = oh0 * gm.stride - gm.pad;   // window top (may be < 0)
    const long xn = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW;
    const int tile_p = min(BP, P - p0);
    // per-thread fragment ownership (as the gather kernel)
    const int mm_a = tid >> 2, kkb = (tid & 3) * 8;
    const int pp_b = tid >> 2;
    const int ow_b = (p0 + pp_b - n * OHW) - (oh0 + pp_b / gm.OW) * gm.OW;
    const int ohl_b = (pp_b / gm.OW) * gm.stride;   // window-row base
    const int iwl_b = ow_b * gm.stride;             // window-col base (pre-pad)
    float va[8];

    f32x4 acc[2][2] = {};
    for (int k0 = ks; k0 < ke; k0 += BK) {
        const int cin0 = k0 / kk2;
        const int cin1 = min(gm.Cin - 1, (k0 + BK - 1) / kk2);
        const int nch = cin1 - cin0 + 1;
        // stage the window slab (coalesced along the input width)
        const int wtot = nch * rows_in * gm.W;
        for (int e = tid; e < wtot; e += 256) {
            const int ww = e % gm.W;
            const int rr = (e / gm.W) % rows_in;
            const int cc = e / (gm.W * rows_in);
            const int ih = ih0 + rr;
            win[cc][rr][ww + gm.pad] =
                (ih >= 0 && ih < gm.H)
                    ? ld_f32(x + xn + (long)(cin0 + cc) * HW + ih * gm.W + ww)
                    : 0.f;
        }
        // zero the horizontal pad columns
        for (int e = tid; e < nch * rows_in * gm.pad * 2; e += 256) {
            const int side = e & 1;
            const int pe = e >> 1;
            const int pcol = pe % gm.pad;
            const int rr = (pe / gm.pad) % rows_in;
            const int cc = pe / (gm.pad * rows_in);
            win[cc][rr][side ? gm.pad + gm.W + pcol : pcol] = 0.f;
        }
        // A tile (weights, coalesced fp32)
        {
            const int m = m0 + mm_a;
            const float* wrow = w + (long)(g * gm.Cout + m) * K + k0 + kkb;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + kkb + j;
                va[j] = (m < M && k < K) ? wrow[j] : 0.f;
            }
            st8_lds(&a_lds[mm_a][kkb], va);
        }
        __syncthreads();
        // B tile built from the LDS window
        {
            float vb[8];
            int k = k0 + kkb;
            int cin = k / kk2, r = k - cin * kk2;
            int kh = r / gm.khw, kw = r - kh * gm.khw;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                vb[j] = (k + j < K && pp_b < tile_p)
                            ? win[cin - cin0][ohl_b + kh][iwl_b + kw]
                            : 0.f;
                if (++kw == gm.khw) {
                    kw = 0;
                    if (++kh == gm.khw) {
                        kh = 0;
                        ++cin;
                    }
                }
            }
            st8_lds(&b_lds[pp_b][kkb], vb);
        }
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        __syncthreads();
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cout * OHW;
    const long yb0 = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW
                     + (p0 - n * OHW);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int pp = wp + fp * 16 + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (m < M && pp < tile_p)
                    fwd_store(acc[fm][fp][r], yb0 + pp + (long)m * OHW,
                              g * gm.Cout + m, bias, residual, y, partial,
                              slab, splitk);
            }
        }
}

// ----------------------------------- staged stride-1 bwd-data (LDS window)
// Same idea as conv_fwd_staged_kernel: a BP-pixel dx tile within one
// sample spanning whole input rows has a dense dy window; stage it
// coalesced and build the transposed-conv patch matrix from LDS.
template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_bwd_data_staged_kernel(const T* __restrict__ dy,
                            const float* __restrict__ w, T* __restrict__ dx,
                            float* __restrict__ partial, ConvGeom gm,
                            int splitk) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ float win[WIN_CH][WIN_ROWS][WIN_W];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int c0 = tc.row0, q0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int J = gm.Cout * kk2;
    const int K = gm.Cin * kk2;
    const int HW = gm.H * gm.W;
    const int OHW = gm.OH * gm.OW;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int njc = ((J + BK - 1) / BK + splitk - 1) / splitk;
    const int js = sp * njc * BK;
    const int je = min(J, js + njc * BK);
    // tile geometry (stride 1: OH=H, OW=W)
    const int n = q0 / HW;
    const int ih0 = (q0 - n * HW) / gm.W;
    const int nrow_in = BP / gm.W;
    const int rows_w = nrow_in + gm.khw - 1;
    const int ohs_min = ih0 + gm.pad - (gm.khw - 1);
    const long dyn = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW;
    const int cc_a = tid >> 2, jjb = (tid & 3) * 8;
    // this thread's pixel for the B build
    const int iwl = (q0 + cc_a - n * HW) - (ih0 + cc_a / gm.W) * gm.W;
    const int rowl = (cc_a / gm.W) + (gm.khw - 1);   // ih - ih0 + (khw-1)
    float va[8];

    f32x4 acc[2][2] = {};
    for (int j0 = js; j0 < je; j0 += BK) {
        const int co0 = j0 / kk2;
        const int co1 = min(gm.Cout - 1, (j0 + BK - 1) / kk2);
        const int nch = co1 - co0 + 1;
        const int wtot = nch * rows_w * gm.OW;
        for (int e = tid; e < wtot; e += 256) {
            const int ww = e % gm.OW;
            const int rr = (e / gm.OW) % rows_w;
            const int cc = e / (gm.OW * rows_w);
            const int ohs = ohs_min + rr;
            win[cc][rr][ww + gm.pad] =
                (ohs >= 0 && ohs < gm.OH)
                    ? ld_f32(dy + dyn + (long)(co0 + cc) * OHW
                             + ohs * gm.OW + ww)
                    : 0.f;
        }
        for (int e = tid; e < nch * rows_w * gm.pad * 2; e += 256) {
            const int side = e & 1;
            const int pe = e >> 1;
            const int pcol = pe % gm.pad;
            const int rr = (pe / gm.pad) % rows_w;
            const int cc = pe / (gm.pad * rows_w);
            win[cc][rr][side ? gm.pad + gm.OW + pcol : pcol] = 0.f;
        }
        {   // A tile: w[g*Cout + cout][c*kk2 + r] rows=c
            const int c = c0 + cc_a;
            int j = j0 + jjb;
            int cout = j / kk2, r = j - cout * kk2;
            int kh = r / gm.khw, kw = r - kh * gm.khw;
#pragma unroll
            for (int j8 = 0; j8 < 8; ++j8) {
                va[j8] = (c < gm.Cin && j + j8 < J)
                             ? w[(long)(g * gm.Cout + cout) * K + c * kk2
                                 + kh * gm.khw + kw]
                             : 0.f;
                if (++kw == gm.khw) {
                    kw = 0;
                    if (++kh == gm.khw) {
                        kh = 0;
                        ++cout;
                    }
                }
            }
            st8_lds(&a_lds[cc_a][jjb], va);
        }
        __syncthreads();
        {   // B tile from window: row = rowl - kh, col = iwl + 2*pad? no:
            // needed dy[ohs = ih + pad - kh][ows = iw + pad - kw];
            // win row = ohs - ohs_min = rowl - kh; win col = ows + pad
            //         = iwl + 2*pad - kw... stored col = ows + pad where
            // ows = iw + pad - kw -> col = iw + 2*pad - kw
            float vb[8];
            int j = j0 + jjb;
            int cout = j / kk2, r = j - cout * kk2;
            int kh = r / gm.khw, kw = r - kh * gm.khw;
#pragma unroll
            for (int j8 = 0; j8 < 8; ++j8) {
                vb[j8] = (j + j8 < J)
                             ? win[cout - co0][rowl - kh]
                                  [iwl + 2 * gm.pad - kw]
                             : 0.f;
                if (++kw == gm.khw) {
                    kw = 0;
                    if (++kh == gm.khw) {
                        kh = 0;
                        ++cout;
                    }
                }
            }
            st8_lds(&b_lds[cc_a][jjb], vb);
        }
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        __syncthreads();
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cin * HW;
    const long xb0 = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW
                     + (q0 - n * HW);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int qq = wp + fp * 16 + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (c < gm.Cin) {
                    const long off = xb0 + qq + (long)c * HW;
                    if (splitk == 1)
                        st_f32(dx + off, acc[fm][fp][r]);
                    else
                        partial[slab + off] = acc[fm][fp][r];
                }
            }
        }
}

// -------------------------------------- staged bwd-weight (x window in LDS)
// The k-tile (hence the input-channel span) is FIXED per block, so the x
// window only advances rows as the P loop walks output rows: stage the
// dense (channels x rows x width) slab per p-step and build the patch
// tile from LDS.  Channels per 64-wide k-tile: ceil(64/9)+1 <= 9.
constexpr int WWIN_CH = 9;

template <typename T, typename TA, typename TB>
__global__ void __launch_bounds__(256)
conv_bwd_weight_staged_kernel(const T* __restrict__ dy,
                              const T* __restrict__ x,
                              float* __restrict__ out, ConvGeom gm,
                              int splitp) {
    __shared__ TA a_lds[BM][LDK];
    __shared__ TB b_lds[BP][LDK];
    __shared__ float win[WWIN_CH][WIN_ROWS][WIN_W];
    __shared__ long t_dyb[BK];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, k0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int pchunk0 = (P + splitp - 1) / splitp;
    const int pchunk = ((pchunk0 + BK - 1) / BK) * BK;  // BK-aligned chunks
    const int pstart = sp * pchunk;
    const int pend = min(P, pstart + pchunk);
    const int cin0 = k0 / kk2;
    const int nch = min(gm.Cin - 1, (k0 + BP - 1) / kk2) - cin0 + 1;
    const int nrow_out = BK / gm.OW;          // 32 pixels per p-step
    const int rows_in = (nrow_out - 1) * gm.stride + gm.khw;
    // per-thread B ownership: fixed k, 8 consecutive pixels
    const int kk_b = (tid >> 2) & 63, ppb = (tid & 3) * 8;
    const int k_b = k0 + kk_b;
    int cin_b = 0, kh_b = 0, kw_b = 0;
    if (k_b < K) {
        cin_b = k_b / kk2;
        const int r = k_b - cin_b * kk2;
        kh_b = r / gm.khw;
        kw_b = r - kh_b * gm.khw;
    }
    const int mm_a = tid >> 2;   // A rows (dy), 8 consecutive p via t_dyb

    f32x4 acc[2][2] = {};
    for (int p0 = pstart; p0 < pend; p0 += BK) {
        __syncthreads();
        const int n = p0 / OHW;
        const int oh0 = (p0 - n * OHW) / gm.OW;
        const int ih0 = oh0 * gm.stride - gm.pad;
        const long xn = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW;
        if (tid < BK) {
            const int p = p0 + tid;
            t_dyb[tid] = (p < pend && p < P)
                             ? ((long)n * gm.G * gm.Cout
                                + (long)g * gm.Cout) * OHW + (p - n * OHW)
                             : -1;
        }
        const int wtot = nch * rows_in * gm.W;
        for (int e = tid; e < wtot; e += 256) {
            const int ww = e % gm.W;
            const int rr = (e / gm.W) % rows_in;
            const int cc = e / (gm.W * rows_in);
            const int ih = ih0 + rr;
            win[cc][rr][ww + gm.pad] =
                (ih >= 0 && ih < gm.H)
                    ? ld_f32(x + xn + (long)(cin0 + cc) * HW + ih * gm.W + ww)
                    : 0.f;
        }
        for (int e = tid; e < nch * rows_in * gm.pad * 2; e += 256) {
            const int side = e & 1;
            const int pe = e >> 1;
            const int pcol = pe % gm.pad;
            const int rr = (pe / gm.pad) % rows_in;
            const int cc = pe / (gm.pad * rows_in);
            win[cc][rr][side ? gm.pad + gm.W + pcol : pcol] = 0.f;
        }
        __syncthreads();
        {   // A tile: dy rows (coalesced via t_dyb)
            const int m = m0 + mm_a;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pp = ppb + j;
                v[j] = (m < M && t_dyb[pp] >= 0)
                           ? ld_f32(dy + t_dyb[pp] + (long)m * OHW) : 0.f;
            }
            st8_lds(&a_lds[mm_a][ppb], v);
        }
        {   // B tile from the window: 8 consecutive pixels of one k
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pp = ppb + j;
                v[j] = 0.f;
                if (k_b < K && p0 + pp < pend) {
                    const int ohl = (pp / gm.OW) * gm.stride;
                    const int owp = pp - (pp / gm.OW) * gm.OW;
                    v[j] = win[cin_b - cin0][ohl + kh_b]
                              [owp * gm.stride + kw_b];
                }
            }
            st8_lds(&b_lds[kk_b][ppb], v);
        }
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile2<TA, TB>(
                    &a_lds[wm + fm * 16 + (l & 15)][0],
                    &b_lds[wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
    }
    __syncthreads();
    const long GK = (long)gm.G * gm.Cout * K;
    float* slab = out + (long)sp * GK;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                const int k = k0 + wp + fp * 16 + (l & 15);
                if (m < M && k < K)
                    slab[(long)(g * gm.Cout + m) * K + k] = acc[fm][fp][r];
            }
}

// ------------------------------------------------ resident-window kernels
// The staged kernels above restage their window on every k-step and pay
// runtime div/mod per staged element; they are bound by VALU issue, not by
// memory (profiles/NOTES.md, "resident window").  The resident variants
// stage the window ONCE per block for the block's whole K/J slice, as raw T
// (no float round trip), and turn every k -> (channel, kh, kw) decode into
// a per-block offset table built in the prologue, so the k-loop carries no
// integer division: a B element is one LDS read at table[k] + pixel_base.
// Operands, their order and the BK chunking are those of the staged
// kernels, so results are bit-identical (HETEROFL_CONV_RESIDENT=0 routes
// back to them for A/B).
//
// Window layout: rows of `width` elements, each preceded by a WGAP-element
// zero gap; the gap serves as the row's left pad and as the right pad of
// the row before it (pad <= WGAP/2), and one trailing gap closes the last
// row.  Row stride S = width + WGAP keeps rows 16-byte aligned whenever
// `width` allows 16-byte global loads.
constexpr int WGAP = 8;

template <typename T> struct RawOf { typedef float type; };
template <> struct RawOf<__hip_bfloat16> { typedef unsigned short type; };
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ void st8_raw(unsigned short* dst,
                                        const unsigned short* v) {
    u32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        t[j] = (unsigned)v[2 * j] | ((unsigned)v[2 * j + 1] << 16);
    *(u32x4*)dst = t;
}
__device__ __forceinline__ void st8_raw(float* dst, const float* v) {
    st8_lds(dst, v);
}

// Stage nch channels x nrows rows of a dense image (row length `width`,
// channel stride chs) into `win`; window row rr is image row row0 + rr,
// zero-filled outside [0, img_rows).  `vec`: 16-byte loads are legal.
template <typename R>
__device__ __forceinline__ void stage_window(R* win, const R* src, long chs,
                                             int nch, int nrows, int row0,
                                             int img_rows, int width, int S,
                                             bool vec, int tid) {
    constexpr int VE = 16 / (int)sizeof(R);
    const int nrt = nch * nrows;
    if (vec) {
        const int vpr = width / VE;
        const int nvec = nrt * vpr;
#pragma unroll 4
        for (int v = tid; v < nvec; v += 256) {
            const int rowi = v / vpr, wv = v - rowi * vpr;
            const int cc = rowi / nrows, rr = rowi - cc * nrows;
            const int ir = row0 + rr;
            u32x4 val = {0u, 0u, 0u, 0u};
            if (ir >= 0 && ir < img_rows)
                val = *(const u32x4*)(src + (long)cc * chs + ir * width
                                      + wv * VE);
            *(u32x4*)(win + rowi * S + WGAP + wv * VE) = val;
        }
    } else {
        const int ntot = nrt * width;
        for (int e = tid; e < ntot; e += 256) {
            const int rowi = e / width, ww = e - rowi * width;
            const int cc = rowi / nrows, rr = rowi - cc * nrows;
            const int ir = row0 + rr;
            R val = (R)0;
            if (ir >= 0 && ir < img_rows)
                val = src[(long)cc * chs + ir * width + ww];
            win[rowi * S + WGAP + ww] = val;
        }
    }
    for (int i = tid; i < (nrt + 1) * WGAP; i += 256)
        win[(i >> 3) * S + (i & (WGAP - 1))] = (R)0;
}

// flags: bit 0 = window rows take 16-byte loads, bit 1 = weight rows take
// float4 loads (K % 4 == 0, base aligned).  Dynamic LDS: the window, then
// the ushort k-offset table at byte offset tab_bytes (nkc*BK entries).
// Requires P % BP == 0 (the staged route's whole-row tiles).
template <typename T>
__global__ void __launch_bounds__(256)
conv_fwd_resident_kernel(const T* __restrict__ x, const float* __restrict__ w,
                         const float* __restrict__ bias,
                         const T* __restrict__ residual, T* __restrict__ y,
                         float* __restrict__ partial, ConvGeom gm, int splitk,
                         int tab_bytes, int flags) {
    typedef typename RawOf<T>::type R;
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    R* win = (R*)dyn_lds;
    unsigned short* koff = (unsigned short*)(dyn_lds + tab_bytes);
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, p0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int nkc = ((K + BK - 1) / BK + splitk - 1) / splitk;
    const int ks = sp * nkc * BK;
    const int ke = min(K, ks + nkc * BK);
    // tile geometry: one sample, whole output rows
    const int n = p0 / OHW;
    const int oh0 = (p0 - n * OHW) / gm.OW;
    const int nrow_out = BP / gm.OW;
    const int rows_in = (nrow_out - 1) * gm.stride + gm.khw;
    const int ih0 = oh0 * gm.stride - gm.pad;   // window top (may be < 0)
    const long xn = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW;
    const int S = gm.W + WGAP;
    const int mm_a = tid >> 2, kkb = (tid & 3) * 8;
    const int pp_b = tid >> 2;

    // prologue: window for the slice's whole channel span + k-offset table
    const int cin_lo = ks / kk2;
    if (ks < ke) {   // empty split slices stage nothing and write zeros
        const int nch = (ke - 1) / kk2 - cin_lo + 1;
        stage_window<R>(win, (const R*)x + xn + (long)cin_lo * HW, HW, nch,
                        rows_in, ih0, gm.H, gm.W, S, flags & 1, tid);
        for (int i = tid; i < nkc * BK; i += 256) {
            const int k = ks + i;
            int off = 0;
            if (k < ke) {
                const int cin = k / kk2, r = k - cin * kk2;
                const int kh = r / gm.khw, kw = r - kh * gm.khw;
                off = ((cin - cin_lo) * rows_in + kh) * S + kw;
            }
            koff[i] = (unsigned short)off;
        }
    }
    __syncthreads();
    const int pbase = (pp_b / gm.OW) * gm.stride * S + WGAP
                      + (pp_b % gm.OW) * gm.stride - gm.pad;
    const bool m_full = (m0 + BM <= M);
    const float* wrow0 = w + (long)(g * gm.Cout + m0 + mm_a) * K + kkb;

    f32x4 acc[2][2] = {};
    float va[8];
    auto load_a = [&](int k0) {
        const float* wrow = wrow0 + k0;
        if ((flags & 2) && m_full && k0 + BK <= ke) {   // block-uniform
            const f32x4 lo = *(const f32x4*)wrow;
            const f32x4 hi = *(const f32x4*)(wrow + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = lo[j];
                va[4 + j] = hi[j];
            }
        } else {
            const bool mok = (m0 + mm_a < M);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                va[j] = (mok && k0 + kkb + j < ke) ? wrow[j] : 0.f;
        }
    };
    auto build_b = [&](int k0, T* dst) {
        const u32x4 kv = *(const u32x4*)(koff + (k0 - ks) + kkb);
        R vb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int off = (kv[j >> 1] >> ((j & 1) * 16)) & 0xffff;
            vb[j] = win[pbase + off];
        }
        if (k0 + BK > ke) {   // ragged last chunk (ke == K here)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k0 + kkb + j >= ke) vb[j] = (R)0;
        }
        st8_raw((R*)dst, vb);
    };
    // double-buffered k-loop: one barrier per k-step
    if (ks < ke) {
        load_a(ks);
        st8_lds(&a_lds[0][mm_a][kkb], va);
        build_b(ks, &b_lds[0][pp_b][kkb]);
        if (ks + BK < ke) load_a(ks + BK);
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = ks; k0 < ke; k0 += BK) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile<T>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (k0 + BK < ke) {
            st8_lds(&a_lds[cur ^ 1][mm_a][kkb], va);
            build_b(k0 + BK, &b_lds[cur ^ 1][pp_b][kkb]);
            if (k0 + 2 * BK < ke) load_a(k0 + 2 * BK);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cout * OHW;
    const long yb0 = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW
                     + (p0 - n * OHW);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int pp = wp + fp * 16 + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (m < M)
                    fwd_store(acc[fm][fp][r], yb0 + pp + (long)m * OHW,
                              g * gm.Cout + m, bias, residual, y, partial,
                              slab, splitk);
            }
        }
}

// Stride-1 bwd-data mirror: the dy window of the block's whole J slice is
// resident; joff[j] holds the window offset of (cout, kh, kw) with the
// (khw-1-kh, khw-1-kw) flip folded in (so offsets stay non-negative), and
// woff[j] the strided weight offset cout*K + tap.  Dynamic LDS: window,
// int woff table at woff_bytes, ushort joff table at joff_bytes.
template <typename T>
__global__ void __launch_bounds__(256)
conv_bwd_data_resident_kernel(const T* __restrict__ dy,
                              const float* __restrict__ w,
                              T* __restrict__ dx, float* __restrict__ partial,
                              ConvGeom gm, int splitk, int woff_bytes,
                              int joff_bytes, int flags) {
    typedef typename RawOf<T>::type R;
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    R* win = (R*)dyn_lds;
    int* woff = (int*)(dyn_lds + woff_bytes);
    unsigned short* joff = (unsigned short*)(dyn_lds + joff_bytes);
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int c0 = tc.row0, q0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int J = gm.Cout * kk2;
    const int K = gm.Cin * kk2;
    const int HW = gm.H * gm.W;
    const int OHW = gm.OH * gm.OW;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int njc = ((J + BK - 1) / BK + splitk - 1) / splitk;
    const int js = sp * njc * BK;
    const int je = min(J, js + njc * BK);
    // tile geometry (stride 1)
    const int n = q0 / HW;
    const int ih0 = (q0 - n * HW) / gm.W;
    const int nrow_in = BP / gm.W;
    const int rows_w = nrow_in + gm.khw - 1;
    const int ohs_min = ih0 + gm.pad - (gm.khw - 1);
    const long dyn = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW;
    const int S = gm.OW + WGAP;
    const int cc_a = tid >> 2, jjb = (tid & 3) * 8;

    const int co_lo = js / kk2;
    if (js < je) {
        const int nch = (je - 1) / kk2 - co_lo + 1;
        stage_window<R>(win, (const R*)dy + dyn + (long)co_lo * OHW, OHW, nch,
                        rows_w, ohs_min, gm.OH, gm.OW, S, flags & 1, tid);
        for (int i = tid; i < njc * BK; i += 256) {
            const int j = js + i;
            int off = 0, wo = 0;
            if (j < je) {
                const int cout = j / kk2, r = j - cout * kk2;
                const int kh = r / gm.khw, kw = r - kh * gm.khw;
                off = ((cout - co_lo) * rows_w + (gm.khw - 1 - kh)) * S
                      + (gm.khw - 1 - kw);
                wo = cout * K + r;
            }
            joff[i] = (unsigned short)off;
            woff[i] = wo;
        }
    }
    __syncthreads();
    // needed dy[ohs = ih + pad - kh][ows = iw + pad - kw]; window row
    // ohs - ohs_min = ihl + (khw-1-kh), column WGAP + ows
    const int pbase = (cc_a / gm.W) * S + WGAP + (cc_a % gm.W) + gm.pad
                      - (gm.khw - 1);
    const bool c_ok = (c0 + cc_a < gm.Cin);
    const float* wbase = w + (long)g * gm.Cout * K + (long)(c0 + cc_a) * kk2;

    f32x4 acc[2][2] = {};
    float va[8];
    auto load_a = [&](int j0) {
        const int* wo = woff + (j0 - js) + jjb;
        const u32x4 lo = *(const u32x4*)wo;
        const u32x4 hi = *(const u32x4*)(wo + 4);
        if (j0 + BK <= je) {   // block-uniform interior chunk
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                va[j8] = c_ok ? wbase[lo[j8]] : 0.f;
                va[4 + j8] = c_ok ? wbase[hi[j8]] : 0.f;
            }
        } else {
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                va[j8] = (c_ok && j0 + jjb + j8 < je) ? wbase[lo[j8]] : 0.f;
                va[4 + j8] = (c_ok && j0 + jjb + 4 + j8 < je) ? wbase[hi[j8]]
                                                              : 0.f;
            }
        }
    };
    auto build_b = [&](int j0, T* dst) {
        const u32x4 jv = *(const u32x4*)(joff + (j0 - js) + jjb);
        R vb[8];
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int off = (jv[j8 >> 1] >> ((j8 & 1) * 16)) & 0xffff;
            vb[j8] = win[pbase + off];
        }
        if (j0 + BK > je) {
#pragma unroll
            for (int j8 = 0; j8 < 8; ++j8)
                if (j0 + jjb + j8 >= je) vb[j8] = (R)0;
        }
        st8_raw((R*)dst, vb);
    };
    if (js < je) {
        load_a(js);
        st8_lds(&a_lds[0][cc_a][jjb], va);
        build_b(js, &b_lds[0][cc_a][jjb]);
        if (js + BK < je) load_a(js + BK);
    }
    __syncthreads();
    int cur = 0;
    for (int j0 = js; j0 < je; j0 += BK) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile<T>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (j0 + BK < je) {
            st8_lds(&a_lds[cur ^ 1][cc_a][jjb], va);
            build_b(j0 + BK, &b_lds[cur ^ 1][cc_a][jjb]);
            if (j0 + 2 * BK < je) load_a(j0 + 2 * BK);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cin * HW;
    const long xb0 = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW
                     + (q0 - n * HW);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int qq = wp + fp * 16 + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (c < gm.Cin) {
                    const long off = xb0 + qq + (long)c * HW;
                    if (splitk == 1)
                        st_f32(dx + off, acc[fm][fp][r]);
                    else
                        partial[slab + off] = acc[fm][fp][r];
                }
            }
        }
}

// 8 consecutive raw elements held packed (one 16-byte register quad per 8
// bf16, two per 8 fp32)
template <typename R> struct Pack8 { u32x4 v[sizeof(R) / 2]; };

template <typename R>
__device__ __forceinline__ Pack8<R> ld8_pack(const R* p, bool vec) {
    Pack8<R> r;
    if (vec) {
#pragma unroll
        for (int i = 0; i < (int)sizeof(R) / 2; ++i)
            r.v[i] = ((const u32x4*)p)[i];
    } else if constexpr (sizeof(R) == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            r.v[0][j] = (unsigned)p[2 * j] | ((unsigned)p[2 * j + 1] << 16);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            r.v[j >> 2][j & 3] = __float_as_uint(p[j]);
    }
    return r;
}
template <typename R>
__device__ __forceinline__ void st8_pack(R* dst, const Pack8<R>& r) {
#pragma unroll
    for (int i = 0; i < (int)sizeof(R) / 2; ++i) ((u32x4*)dst)[i] = r.v[i];
}

// bwd-weight: the channel span is fixed per block and every p-step covers
// whole output rows of one sample, so the x window is staged once per
// SAMPLE SEGMENT of the block's p-chunk (not once per 32-pixel step) and a
// p-step only moves the window row base.  The p-loop carries no division:
// (n, hw, oh) advance as counters, each thread's 8 pixel offsets are
// prologue constants, and the dy tile is one packed 16-byte-per-8-pixels
// copy (all 32 pixels of a step are live: chunks and P are BK-aligned).
// flags: bit 0 = x rows take 16-byte loads, bit 1 = dy takes them.
template <typename T>
__global__ void __launch_bounds__(256)
conv_bwd_weight_resident_kernel(const T* __restrict__ dy,
                                const T* __restrict__ x,
                                float* __restrict__ out, ConvGeom gm,
                                int splitp, int flags) {
    typedef typename RawOf<T>::type R;
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    R* win = (R*)dyn_lds;
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, k0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int pchunk0 = (P + splitp - 1) / splitp;
    const int pchunk = ((pchunk0 + BK - 1) / BK) * BK;  // BK-aligned chunks
    const int pstart = sp * pchunk;
    const int pend = min(P, pstart + pchunk);
    const int cin0 = k0 / kk2;
    const int nch = min(gm.Cin - 1, (k0 + BP - 1) / kk2) - cin0 + 1;
    const int nrow_out = BK / gm.OW;          // output rows per p-step
    const int S = gm.W + WGAP;
    const int step_rows = nrow_out * gm.stride * S;
    // per-thread B ownership: fixed k, 8 consecutive pixels
    const int kk_b = (tid >> 2) & 63, ppb = (tid & 3) * 8;
    const int k_b = k0 + kk_b;
    const bool k_ok = (k_b < K);
    int cin_b = cin0, kh_b = 0, kw_b = 0;
    if (k_ok) {
        cin_b = k_b / kk2;
        const int r = k_b - cin_b * kk2;
        kh_b = r / gm.khw;
        kw_b = r - kh_b * gm.khw;
    }
    int poff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int pp = ppb + j;
        poff[j] = (pp / gm.OW) * gm.stride * S + (pp % gm.OW) * gm.stride;
    }
    // per-thread A ownership: one dy row, the same 8 pixels
    const int mm_a = tid >> 2;
    const bool m_ok = (m0 + mm_a < M);
    const long dy_ns = (long)gm.G * gm.Cout * OHW;
    const R* dyrow = (const R*)dy + ((long)g * gm.Cout + m0 + mm_a) * OHW
                     + ppb;
    const bool dvec = (flags & 2) != 0;
    auto load_a = [&](int n_, int hw_) {
        Pack8<R> r = {};
        if (m_ok) r = ld8_pack<R>(dyrow + (long)n_ * dy_ns + hw_, dvec);
        return r;
    };
    auto build_b = [&](int base, T* dst) {
        R vb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            vb[j] = k_ok ? win[base + poff[j]] : (R)0;
        st8_raw((R*)dst, vb);
    };

    f32x4 acc[2][2] = {};
    // chunk position, advanced by counters from here on
    int n = pstart / OHW;
    int hw = pstart - n * OHW;
    int oh = hw / gm.OW;
    int cur = 0;
    for (int p0 = pstart; p0 < pend;) {
        // one sample segment of the chunk: nst p-steps, one window
        const int seg_px = min(pend - p0, OHW - hw);
        const int nst = seg_px / BK;
        const int nrows = (nst * nrow_out - 1) * gm.stride + gm.khw;
        const long xn = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin + cin0)
                        * HW;
        stage_window<R>(win, (const R*)x + xn, HW, nch, nrows,
                        oh * gm.stride - gm.pad, gm.H, gm.W, S, flags & 1,
                        tid);
        __syncthreads();
        const int kbase = ((cin_b - cin0) * nrows + kh_b) * S + WGAP + kw_b
                          - gm.pad;
        Pack8<R> ra = load_a(n, hw);
        st8_pack((R*)&a_lds[cur][mm_a][ppb], ra);
        build_b(kbase, &b_lds[cur][kk_b][ppb]);
        if (nst > 1) ra = load_a(n, hw + BK);
        __syncthreads();
        for (int t = 0; t < nst; ++t) {
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fp = 0; fp < 2; ++fp)
                    acc[fm][fp] = mfma_tile<T>(
                        &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                        &b_lds[cur][wp + fp * 16 + (l & 15)][0],
                        acc[fm][fp]);
            if (t + 1 < nst) {
                st8_pack((R*)&a_lds[cur ^ 1][mm_a][ppb], ra);
                build_b(kbase + (t + 1) * step_rows,
                        &b_lds[cur ^ 1][kk_b][ppb]);
                if (t + 2 < nst) ra = load_a(n, hw + (t + 2) * BK);
            }
            __syncthreads();
            cur ^= 1;
        }
        p0 += seg_px;
        hw += seg_px;
        oh += nst * nrow_out;
        if (hw == OHW) {
            hw = 0;
            oh = 0;
            ++n;
        }
    }
    const long GK = (long)gm.G * gm.Cout * K;
    float* slab = out + (long)sp * GK;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                const int k = k0 + wp + fp * 16 + (l & 15);
                if (m < M && k < K)
                    slab[(long)(g * gm.Cout + m) * K + k] = acc[fm][fp][r];
            }
}

// --------------------------------------------------- tabled gather kernels
// The gather kernels above decode every loaded element's reduction index
// (k -> cin, kh, kw; j -> cout, kh, kw) and bounds-test it with four
// compares inside the k-loop; their loop bodies are ~500-1400 instructions
// around four MFMAs (profiles/NOTES.md, "tabled gather").  None of that
// depends on data.  The tabled variants build, once per block:
//   - a reduction-index table for the block's own slice: per entry the
//     element's offset relative to the pixel base and its tap index, packed
//     (offset << 4) | tap; tap 15 marks an entry past the slice end;
//   - per pixel a tap-validity mask (bit tap = that tap lands inside the
//     image), next to the pixel base;
//   - a block-uniform flag: every tap of every pixel of the tile is valid,
//     so interior chunks skip the mask test altogether.
// An element is then `(mask >> tap) & 1 ? src[base + offset] : 0`.  Loads
// stay raw T (no float round trip).  Operands, their K/J/P order, the BK
// chunking, the split rules and the wave-to-quadrant mapping are those of
// the gather kernels, so results are bit-identical (HETEROFL_CONV_TABLED=0
// routes back to them for A/B).  bf16 and fp32 only; fp8 stays on the old
// kernels, and so does any slice whose table exceeds the capacities below.
// The reduction tables live in dynamic LDS sized by the slice (4 bytes per
// entry fwd, 8 bwd-data), so a short slice does not pay for the capacity.
// The flagship's largest slices: 576 entries (layer 4 with 6-10 full-width
// clients in the group, split 8) and 1024 (the 16x16 stride-2 bwd-data,
// unsplit from 7 clients on); its bwd-weight chunks are at most 160 pixels.
constexpr int TAB_CAP = 1024;       // k / j entries per slice (32 BK-chunks)
constexpr int PIX_TAB_CAP = 256;    // bwd-weight: pixels per p-chunk
constexpr int TAP_NONE = 15;        // table entry past the slice end

// one gathered raw element: entry = (offset << 4) | tap, offset signed
template <typename R>
__device__ __forceinline__ R gather_elem(const R* src, long base, int entry,
                                         unsigned mask) {
    return ((mask >> (entry & 15)) & 1u) ? src[base + (entry >> 4)] : (R)0;
}

// flags: bit 1 = weight rows take float4 loads (K % 4 == 0, base aligned).
template <typename T>
__global__ void __launch_bounds__(256)
conv_fwd_tabled_kernel(const T* __restrict__ x, const float* __restrict__ w,
                       const float* __restrict__ bias,
                       const T* __restrict__ residual, T* __restrict__ y,
                       float* __restrict__ partial, ConvGeom gm, int splitk,
                       int flags) {
    typedef typename RawOf<T>::type R;
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    int* ktab = (int*)dyn_lds;          // nkc * BK entries
    __shared__ long t_ybase[BP];
    const TileCoord tc = tile_coord(gm.G);
    const int g = tc.g, sp = tc.sp;
    const int m0 = tc.row0, p0 = tc.col0;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int tid = tc.tid, l = tc.l, wm = tc.wm, wp = tc.wp;
    const int nkc = ((K + BK - 1) / BK + splitk - 1) / splitk;
    const int ks = sp * nkc * BK;
    const int ke = min(K, ks + nkc * BK);
    const int mm_a = tid >> 2, kkb = (tid & 3) * 8;
    const int pp_b = tid >> 2;

    // prologue: this thread's pixel (base + tap mask), the k table
    long xbase = 0;
    unsigned mask = 0;
    {
        const int p = p0 + pp_b;
        if (p < P) {
            const int n = p / OHW, hw = p - n * OHW;
            const int oh = hw / gm.OW, ow = hw - oh * gm.OW;
            const int ihb = oh * gm.stride - gm.pad;
            const int iwb = ow * gm.stride - gm.pad;
            xbase = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin) * HW
                    + ihb * gm.W + iwb;
            for (int kh = 0; kh < gm.khw; ++kh)
                for (int kw = 0; kw < gm.khw; ++kw) {
                    const int ih = ihb + kh, iw = iwb + kw;
                    if (ih >= 0 && ih < gm.H && iw >= 0 && iw < gm.W)
                        mask |= 1u << (kh * gm.khw + kw);
                }
            if ((tid & 3) == 0)
                t_ybase[pp_b] = ((long)n * gm.G * gm.Cout
                                 + (long)g * gm.Cout) * OHW + hw;
        } else if ((tid & 3) == 0) {
            t_ybase[pp_b] = -1;
        }
    }
    for (int i = tid; i < nkc * BK; i += 256) {
        const int k = ks + i;
        int e = TAP_NONE;
        if (k < ke) {
            const int cin = k / kk2, r = k - cin * kk2;
            const int kh = r / gm.khw, kw = r - kh * gm.khw;
            e = ((cin * HW + kh * gm.W + kw) << 4) | r;
        }
        ktab[i] = e;
    }
    // (also the barrier that publishes ktab and t_ybase)
    const bool interior = __syncthreads_and(mask == (1u << kk2) - 1u);
    const bool m_full = (m0 + BM <= M);
    const float* wrow0 = w + (long)(g * gm.Cout + m0 + mm_a) * K + kkb;
    const R* xr = (const R*)x;

    f32x4 acc[2][2] = {};
    float va[8];
    R vb[8];
    auto load_regs = [&](int k0) {
        const float* wrow = wrow0 + k0;
        const bool full = (k0 + BK <= ke);           // block-uniform
        if ((flags & 2) && m_full && full) {
            const f32x4 lo = *(const f32x4*)wrow;
            const f32x4 hi = *(const f32x4*)(wrow + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = lo[j];
                va[4 + j] = hi[j];
            }
        } else {
            const bool mok = (m0 + mm_a < M);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                va[j] = (mok && k0 + kkb + j < ke) ? wrow[j] : 0.f;
        }
        const int* te = ktab + (k0 - ks) + kkb;
        const u32x4 lo = *(const u32x4*)te;
        const u32x4 hi = *(const u32x4*)(te + 4);
        if (interior && full) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vb[j] = xr[xbase + ((int)lo[j] >> 4)];
                vb[4 + j] = xr[xbase + ((int)hi[j] >> 4)];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vb[j] = gather_elem<R>(xr, xbase, (int)lo[j], mask);
                vb[4 + j] = gather_elem<R>(xr, xbase, (int)hi[j], mask);
            }
        }
    };
    // double-buffered k-loop: one barrier per k-step, tile t+1's loads in
    // flight across tile t's MFMA phase (as conv_fwd_kernel)
    if (ks < ke) {
        load_regs(ks);
        st8_lds(&a_lds[0][mm_a][kkb], va);
        st8_raw((R*)&b_lds[0][pp_b][kkb], vb);
        if (ks + BK < ke) load_regs(ks + BK);
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = ks; k0 < ke; k0 += BK) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile<T>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (k0 + BK < ke) {
            st8_lds(&a_lds[cur ^ 1][mm_a][kkb], va);
            st8_raw((R*)&b_lds[cur ^ 1][pp_b][kkb], vb);
            if (k0 + 2 * BK < ke) load_regs(k0 + 2 * BK);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cout * OHW;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int pp = wp + fp * 16 + (l & 15);
            const long yb = t_ybase[pp];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (m < M && yb >= 0)
                    fwd_store(acc[fm][fp][r], yb + (long)m * OHW,
                              g * gm.Cout + m, bias, residual, y, partial,
                              slab, splitk);
            }
        }
}

// bwd-data, both gather routes.  S2 = the parity-class tiling of
// conv_bwd_data_s2_kernel (table built from the class's compressed tap
// list, tap index = position in that list, at most 4); otherwise the
// any-geometry kernel, stride 1 or 2.  For stride 2 there a pixel's live
// taps are those of its own parity, and for a live tap
// oh = (ih + pad - kh) / 2 = (ih + pad) / 2 - (kh >> 1), so the per-tap
// part still separates from the pixel base; the parity test lives in the
// pixel's mask.  jtab: (dy offset << 4) | tap, offset signed; wtab: the
// strided weight offset cout*K + tap (as the resident kernel's woff).
template <typename T, bool S2>
__device__ __forceinline__ void
conv_bwd_data_tabled_body(const T* __restrict__ dy,
                          const float* __restrict__ w, T* __restrict__ dx,
                          float* __restrict__ partial, const ConvGeom& gm,
                          int splitk, int nyp) {
    typedef typename RawOf<T>::type R;
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    __shared__ long t_xbase[BP];
    const int g = blockIdx.z % gm.G;
    const int sp = blockIdx.z / gm.G;
    const int c0 = blockIdx.x * BM;
    const int cls = S2 ? blockIdx.y / nyp : 0;
    const int q0 = (blockIdx.y - cls * nyp) * BP;
    const int ph = cls >> 1, pw = cls & 1;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int HW = gm.H * gm.W;
    const int OHW = gm.OH * gm.OW;
    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int wm = (wave >> 1) * 32;
    const int wp = (wave & 1) * 32;
    const int cc_a = tid >> 2, jjb = (tid & 3) * 8;
    // the tap list: S2 = taps of this parity class, else all of them
    int nkh = gm.khw, nkw = gm.khw;
    if (S2) {
        nkh = nkw = 0;
        for (int k = 0; k < gm.khw; ++k) {
            nkh += ((ph + gm.pad - k) & 1) == 0;
            nkw += ((pw + gm.pad - k) & 1) == 0;
        }
    }
    const int tap2 = nkh * nkw;
    const int J = gm.Cout * tap2;
    const int njc = ((J + BK - 1) / BK + splitk - 1) / splitk;
    const int js = sp * njc * BK;
    const int je = min(J, js + njc * BK);
    int* jtab = (int*)dyn_lds;          // njc * BK entries each
    int* wtab = jtab + njc * BK;

    // prologue: this thread's pixel (base + tap mask), the j tables
    long dybase = 0;
    unsigned mask = 0;
    if (S2) {
        const int H2 = gm.H >> 1, W2 = gm.W >> 1;
        const int HW2 = H2 * W2;
        const int q = q0 + cc_a;
        if (q < gm.N * HW2) {
            const int n = q / HW2, hw2 = q - n * HW2;
            const int ih2 = hw2 / W2, iw2 = hw2 - ih2 * W2;
            dybase = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW
                     + ih2 * gm.OW + iw2;
            int a = 0;
            for (int kh = 0; kh < gm.khw; ++kh) {
                if ((ph + gm.pad - kh) & 1) continue;
                const int oh = ih2 + ((ph + gm.pad - kh) >> 1);
                int b = 0;
                for (int kw = 0; kw < gm.khw; ++kw) {
                    if ((pw + gm.pad - kw) & 1) continue;
                    const int ow = iw2 + ((pw + gm.pad - kw) >> 1);
                    if (oh >= 0 && oh < gm.OH && ow >= 0 && ow < gm.OW)
                        mask |= 1u << (a * nkw + b);
                    ++b;
                }
                ++a;
            }
            if ((tid & 3) == 0)
                t_xbase[cc_a] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin)
                                    * HW
                                + (2 * ih2 + ph) * gm.W + (2 * iw2 + pw);
        } else if ((tid & 3) == 0) {
            t_xbase[cc_a] = -1;
        }
    } else {
        const int q = q0 + cc_a;
        if (q < gm.N * HW) {
            const int n = q / HW, hw = q - n * HW;
            const int ih = hw / gm.W, iw = hw - ih * gm.W;
            const int sh = gm.stride - 1;           // stride is 1 or 2
            const int ohp = ih + gm.pad, owp = iw + gm.pad;
            dybase = ((long)n * gm.G * gm.Cout + (long)g * gm.Cout) * OHW
                     + (ohp >> sh) * gm.OW + (owp >> sh);
            for (int kh = 0; kh < gm.khw; ++kh)
                for (int kw = 0; kw < gm.khw; ++kw) {
                    const int ohs = ohp - kh, ows = owp - kw;
                    if (ohs < 0 || ows < 0) continue;
                    if (((ohs | ows) & sh) != 0) continue;   // parity
                    if ((ohs >> sh) < gm.OH && (ows >> sh) < gm.OW)
                        mask |= 1u << (kh * gm.khw + kw);
                }
            if ((tid & 3) == 0)
                t_xbase[cc_a] = ((long)n * gm.G * gm.Cin + (long)g * gm.Cin)
                                    * HW + hw;
        } else if ((tid & 3) == 0) {
            t_xbase[cc_a] = -1;
        }
    }
    for (int i = tid; i < njc * BK; i += 256) {
        const int j = js + i;
        int e = TAP_NONE, wo = 0;
        if (j < je) {
            const int cout = j / tap2, rr = j - cout * tap2;
            if (S2) {
                // rr-th live (kh, kw) of the class, row-major
                const int a = rr / nkw, b = rr - a * nkw;
                int kh = 0, kw = 0;
                for (int k = 0, s = -1; k < gm.khw; ++k)
                    if (((ph + gm.pad - k) & 1) == 0 && ++s == a) kh = k;
                for (int k = 0, s = -1; k < gm.khw; ++k)
                    if (((pw + gm.pad - k) & 1) == 0 && ++s == b) kw = k;
                e = (cout * OHW + ((ph + gm.pad - kh) >> 1) * gm.OW
                     + ((pw + gm.pad - kw) >> 1)) * 16 + rr;
                wo = cout * K + kh * gm.khw + kw;
            } else {
                const int kh = rr / gm.khw, kw = rr - kh * gm.khw;
                const int sh = gm.stride - 1;
                e = (cout * OHW - (kh >> sh) * gm.OW - (kw >> sh)) * 16 + rr;
                wo = cout * K + rr;
            }
        }
        jtab[i] = e;
        wtab[i] = wo;
    }
    const bool interior = __syncthreads_and(mask == (1u << tap2) - 1u);
    const bool c_ok = (c0 + cc_a < gm.Cin);
    const float* wbase = w + (long)g * gm.Cout * K + (long)(c0 + cc_a) * kk2;
    const R* dyr = (const R*)dy;

    f32x4 acc[2][2] = {};
    float va[8];
    R vb[8];
    auto load_regs = [&](int j0) {
        const int* wo = wtab + (j0 - js) + jjb;
        const u32x4 wlo = *(const u32x4*)wo;
        const u32x4 whi = *(const u32x4*)(wo + 4);
        const int* te = jtab + (j0 - js) + jjb;
        const u32x4 lo = *(const u32x4*)te;
        const u32x4 hi = *(const u32x4*)(te + 4);
        const bool full = (j0 + BK <= je);           // block-uniform
        if (full) {
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                va[j8] = c_ok ? wbase[wlo[j8]] : 0.f;
                va[4 + j8] = c_ok ? wbase[whi[j8]] : 0.f;
            }
        } else {
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                va[j8] = (c_ok && j0 + jjb + j8 < je) ? wbase[wlo[j8]] : 0.f;
                va[4 + j8] = (c_ok && j0 + jjb + 4 + j8 < je)
                                 ? wbase[whi[j8]] : 0.f;
            }
        }
        if (interior && full) {
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                vb[j8] = dyr[dybase + ((int)lo[j8] >> 4)];
                vb[4 + j8] = dyr[dybase + ((int)hi[j8] >> 4)];
            }
        } else {
#pragma unroll
            for (int j8 = 0; j8 < 4; ++j8) {
                vb[j8] = gather_elem<R>(dyr, dybase, (int)lo[j8], mask);
                vb[4 + j8] = gather_elem<R>(dyr, dybase, (int)hi[j8], mask);
            }
        }
    };
    if (js < je) {
        load_regs(js);
        st8_lds(&a_lds[0][cc_a][jjb], va);
        st8_raw((R*)&b_lds[0][cc_a][jjb], vb);
        if (js + BK < je) load_regs(js + BK);
    }
    __syncthreads();
    int cur = 0;
    for (int j0 = js; j0 < je; j0 += BK) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile<T>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (j0 + BK < je) {
            st8_lds(&a_lds[cur ^ 1][cc_a][jjb], va);
            st8_raw((R*)&b_lds[cur ^ 1][cc_a][jjb], vb);
            if (j0 + 2 * BK < je) load_regs(j0 + 2 * BK);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long slab = (long)sp * gm.N * gm.G * gm.Cin * HW;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
            const int qq = wp + fp * 16 + (l & 15);
            const long xb = t_xbase[qq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (c < gm.Cin && xb >= 0) {
                    if (splitk == 1)
                        st_f32(dx + xb + (long)c * HW, acc[fm][fp][r]);
                    else
                        partial[slab + xb + (long)c * HW] = acc[fm][fp][r];
                }
            }
        }
}

template <typename T>
__global__ void __launch_bounds__(256)
conv_bwd_data_tabled_kernel(const T* __restrict__ dy,
                            const float* __restrict__ w, T* __restrict__ dx,
                            float* __restrict__ partial, ConvGeom gm,
                            int splitk) {
    conv_bwd_data_tabled_body<T, false>(dy, w, dx, partial, gm, splitk, 1);
}

template <typename T>
__global__ void __launch_bounds__(256)
conv_bwd_data_s2_tabled_kernel(const T* __restrict__ dy,
                               const float* __restrict__ w,
                               T* __restrict__ dx, float* __restrict__ partial,
                               ConvGeom gm, int splitk, int nyp) {
    conv_bwd_data_tabled_body<T, true>(dy, w, dx, partial, gm, splitk, nyp);
}

// bwd-weight: the pixel table (x base, dy offset, tap mask) covers the
// block's whole p-chunk and is built once; a thread's k is fixed, so its
// offset cin*HW + kh*W + kw and its tap bit are registers.  Tiles are
// double-buffered: one barrier per p-step (the gather kernel crosses four).
// flags: bit 1 = a thread's 8 dy pixels are one aligned 16/32-byte load
// (OHW % 8 == 0, p-chunk % 8 == 0, base aligned: every 8-group then lies in
// one sample and is wholly inside or wholly outside the chunk).
template <typename T>
__global__ void __launch_bounds__(256)
conv_bwd_weight_tabled_kernel(const T* __restrict__ dy,
                              const T* __restrict__ x,
                              float* __restrict__ out, ConvGeom gm,
                              int splitp, int flags) {
    typedef typename RawOf<T>::type R;
    __shared__ T a_lds[2][BM][LDK];
    __shared__ T b_lds[2][BP][LDK];
    __shared__ __align__(16) int t_xb[PIX_TAB_CAP + BK];
    __shared__ __align__(16) int t_dyb[PIX_TAB_CAP + BK];
    __shared__ __align__(16) unsigned short t_mask[PIX_TAB_CAP + BK];
    const int g = blockIdx.z % gm.G;
    const int sp = blockIdx.z / gm.G;
    const int m0 = blockIdx.x * BM;
    const int k0 = blockIdx.y * BP;
    const int kk2 = gm.khw * gm.khw;
    const int K = gm.Cin * kk2;
    const int M = gm.Cout;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int HW = gm.H * gm.W;
    const int pchunk = (P + splitp - 1) / splitp;
    const int pstart = sp * pchunk;
    const int pend = min(P, pstart + pchunk);
    const int npx = max(pend - pstart, 0);
    const int nst = (npx + BK - 1) / BK;
    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int wm = (wave >> 1) * 32;
    const int wp = (wave & 1) * 32;

    // prologue: pixel table of the chunk, padded to whole p-steps
    unsigned full_px = 1;
    for (int i = tid; i < nst * BK; i += 256) {
        const int p = pstart + i;
        int xb = 0, db = -1;
        unsigned mk = 0;
        if (p < pend) {
            const int n = p / OHW, hw = p - n * OHW;
            const int oh = hw / gm.OW, ow = hw - oh * gm.OW;
            const int ihb = oh * gm.stride - gm.pad;
            const int iwb = ow * gm.stride - gm.pad;
            xb = (n * gm.G * gm.Cin + g * gm.Cin) * HW + ihb * gm.W + iwb;
            db = (n * gm.G * gm.Cout + g * gm.Cout) * OHW + hw;
            for (int kh = 0; kh < gm.khw; ++kh)
                for (int kw = 0; kw < gm.khw; ++kw) {
                    const int ih = ihb + kh, iw = iwb + kw;
                    if (ih >= 0 && ih < gm.H && iw >= 0 && iw < gm.W)
                        mk |= 1u << (kh * gm.khw + kw);
                }
        }
        t_xb[i] = xb;
        t_dyb[i] = db;
        t_mask[i] = (unsigned short)mk;
        if (p < pend) full_px &= (mk == (1u << kk2) - 1u);
    }
    // every pixel of the chunk takes every tap and the k-tile is whole:
    // whole p-steps skip the mask test
    const bool interior = __syncthreads_and(full_px) && (k0 + BP <= K);

    // per-thread ownership: row mm (A: dy row m, B: k), 8 consecutive pixels
    const int mm = (tid >> 2) & 63, ppb = (tid & 3) * 8;
    const bool m_ok = (m0 + mm < M);
    const int k_b = k0 + mm;
    const bool k_ok = (k_b < K);
    int koff = 0;
    unsigned kbit = 0;
    if (k_ok) {
        const int cin = k_b / kk2, r = k_b - cin * kk2;
        const int kh = r / gm.khw, kw = r - kh * gm.khw;
        koff = cin * HW + kh * gm.W + kw;
        kbit = 1u << r;
    }
    const R* dyr = (const R*)dy + (long)(m0 + mm) * OHW;
    const R* xr = (const R*)x + koff;
    const bool dvec = (flags & 2) != 0;

    f32x4 acc[2][2] = {};
    Pack8<R> ra;
    R vb[8];
    auto load_regs = [&](int t) {
        const int i0 = t * BK + ppb;
        const u32x4 xlo = *(const u32x4*)(t_xb + i0);
        const u32x4 xhi = *(const u32x4*)(t_xb + i0 + 4);
        if (dvec) {
            ra = Pack8<R>{};
            if (m_ok && i0 < npx)
                ra = ld8_pack<R>(dyr + t_dyb[i0], true);
        } else {
            const u32x4 dlo = *(const u32x4*)(t_dyb + i0);
            const u32x4 dhi = *(const u32x4*)(t_dyb + i0 + 4);
            R va[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = (m_ok && (int)dlo[j] >= 0) ? dyr[(int)dlo[j]] : (R)0;
                va[4 + j] = (m_ok && (int)dhi[j] >= 0) ? dyr[(int)dhi[j]]
                                                       : (R)0;
            }
            if constexpr (sizeof(R) == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    ra.v[0][j] = (unsigned)va[2 * j]
                                 | ((unsigned)va[2 * j + 1] << 16);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    ra.v[j >> 2][j & 3] = __float_as_uint(va[j]);
            }
        }
        if (interior && (t + 1) * BK <= npx) {        // block-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vb[j] = xr[(int)xlo[j]];
                vb[4 + j] = xr[(int)xhi[j]];
            }
        } else {
            const u32x4 mv = *(const u32x4*)(t_mask + i0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned mk = (mv[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                const int xb = (int)(j < 4 ? xlo[j & 3] : xhi[j & 3]);
                vb[j] = (mk & kbit) ? xr[xb] : (R)0;
            }
        }
    };
    if (nst > 0) {
        load_regs(0);
        st8_pack((R*)&a_lds[0][mm][ppb], ra);
        st8_raw((R*)&b_lds[0][mm][ppb], vb);
        if (nst > 1) load_regs(1);
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nst; ++t) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fp = 0; fp < 2; ++fp)
                acc[fm][fp] = mfma_tile<T>(
                    &a_lds[cur][wm + fm * 16 + (l & 15)][0],
                    &b_lds[cur][wp + fp * 16 + (l & 15)][0], acc[fm][fp]);
        if (t + 1 < nst) {
            st8_pack((R*)&a_lds[cur ^ 1][mm][ppb], ra);
            st8_raw((R*)&b_lds[cur ^ 1][mm][ppb], vb);
            if (t + 2 < nst) load_regs(t + 2);
        }
        __syncthreads();
        cur ^= 1;
    }
    const long GK = (long)gm.G * gm.Cout * K;
    float* slab = out + (long)sp * GK;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                const int k = k0 + wp + fp * 16 + (l & 15);
                if (m < M && k < K)
                    slab[(long)(g * gm.Cout + m) * K + k] = acc[fm][fp][r];
            }
}

// ------------------------------------------------------------ host layer
// Deciding is separate from launching.  plan_fwd / plan_bwd_data /
// plan_bwd_weight are pure functions of (geometry, element size, fp8 flag)
// and the HETEROFL_CONV_* switches; each conv_* entry point below selects a
// kernel from its plan and launches once.  conv_plan() hands the same plans
// to Python so a test can pin which kernel and split a shape takes.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <tuple>
#include <type_traits>

// target concurrent-block count for the split-K/split-P decompositions
// (tunable: HETEROFL_CONV_SPLIT_TARGET, default 1024 = 4 blocks/CU)
static int split_target() {
    static int t = [] {
        const char* e = std::getenv("HETEROFL_CONV_SPLIT_TARGET");
        return e ? std::atoi(e) : 1024;
    }();
    return t;
}

// resident-window routing.  HETEROFL_CONV_RESIDENT=0 (read on every call,
// so one process can flip it) routes back to the staged kernels.  A slice
// is resident only while static + dynamic LDS stays under the cap.  The
// cap is 64 KB, the most a launch gets without a function attribute:
// measured (profiles/convbench_resident.txt, shapes X96/X128), slices
// between 53 KB (3 blocks/CU of 160 KB) and 64 KB (2 blocks/CU) still run
// 2.4-2.7x faster resident than staged, so the lower-occupancy resident
// kernel beats the fallback (HETEROFL_CONV_RESIDENT_LDS lowers the cap
// for sweeps).
static bool resident_on() {
    const char* e = std::getenv("HETEROFL_CONV_RESIDENT");
    return !(e && e[0] == '0');
}
static int resident_lds_cap() {
    static int c = [] {
        const char* e = std::getenv("HETEROFL_CONV_RESIDENT_LDS");
        const int v = e ? std::atoi(e) : 65536;
        return v > 65536 ? 65536 : v;
    }();
    return c;
}
// tabled gather routing.  HETEROFL_CONV_TABLED=0 (read on every call)
// routes the gather routes back to the untabled kernels.  A slice is tabled
// only while its table fits the kernel's capacity (TAB_CAP
// reduction entries per slice, PIX_TAB_CAP pixels per p-chunk),
// the tap index fits 4 bits with 15 spare (khw <= 3), and the packed
// offsets fit an int; anything else, and every fp8 launch, takes the
// untabled kernel.
static bool tabled_on() {
    const char* e = std::getenv("HETEROFL_CONV_TABLED");
    return !(e && e[0] == '0');
}
static bool aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}
// LDS need of one resident fwd / bwd-data launch (bytes); chunks =
// BK-chunks per slice, tap2 = khw*khw, nchan = channels of the staged
// tensor, width = its row
static bool resident_window_fits(int chunks, int tap2, int nchan, int rows,
                                 int width, int esz, int tab_entry_bytes,
                                 int* win_bytes) {
    const int nch_max = std::min(nchan, (chunks * BK - 1) / tap2 + 2);
    const long welems = (long)nch_max * rows * (width + WGAP) + WGAP;
    if (welems >= 65536) return false;   // ushort offsets
    *win_bytes = (int)((welems * esz + 15) / 16 * 16);
    const int stat = 2 * (BM + BP) * LDK * esz;
    return stat + *win_bytes + chunks * BK * tab_entry_bytes
           <= resident_lds_cap();
}

static int cdiv(int a, int b) { return (a + b - 1) / b; }

static ConvGeom conv_geom(int64_t G, int64_t N, int64_t Cin, int64_t H,
                          int64_t W, int64_t Cout, int64_t khw,
                          int64_t stride, int64_t pad) {
    ConvGeom gm;
    gm.G = (int)G;
    gm.N = (int)N;
    gm.H = (int)H;
    gm.W = (int)W;
    gm.Cin = (int)Cin;
    gm.Cout = (int)Cout;
    gm.khw = (int)khw;
    gm.stride = (int)stride;
    gm.pad = (int)pad;
    TORCH_CHECK(gm.khw > 0 && gm.stride > 0 && gm.H + 2 * gm.pad >= gm.khw
                && gm.W + 2 * gm.pad >= gm.khw, "bad conv geometry");
    gm.OH = (gm.H + 2 * gm.pad - gm.khw) / gm.stride + 1;
    gm.OW = (gm.W + 2 * gm.pad - gm.khw) / gm.stride + 1;
    return gm;
}

enum Route { GATHER, GATHER_S2, STAGED, RESIDENT };

struct ConvPlan {
    Route route;
    bool fp8;       // gather kernels only: the e4m3/e5m2 tile instantiation
    bool tabled;    // gather routes only: the tabled kernel of the route
    int tab_lds;    // tabled fwd / bwd-data launch: dynamic LDS of its tables
    int split;      // split-K (fwd, bwd-data) or split-P (bwd-weight)
    dim3 grid;
    int dyn_lds;    // resident launch: dynamic LDS bytes
    int tab0, tab1; // resident launch: byte offsets of its tables in there
    int nyp;        // gather_s2: pixel tiles per parity class
};

// Split of the fwd (K) and bwd-data (J) reduction over `tiles` output
// tiles.  Same rule as bwdW (measured, L3): short reductions with enough
// tiles run best unsplit — the split's partial-write + reduce traffic beats
// the extra parallelism.
static int split_reduction(int red, int tiles) {
    const int chunks = cdiv(red, BK);
    int split = 1;
    if (red > 1024 || tiles < 512)
        while (tiles * split < split_target() && split * 2 <= chunks / 2)
            split *= 2;
    return split;
}

// fp8 tiles exist for bf16 tensors only (esz == 2).  With fp8 set on fp32
// tensors the directions differ, and that is kept as it always was: fwd
// leaves the window kernels for the plain fp32 gather kernel, bwd-data
// leaves only the resident kernel (for the staged one), bwd-weight ignores
// the flag.
static ConvPlan plan_fwd(const ConvGeom& gm, int esz, bool fp8) {
    const int tap2 = gm.khw * gm.khw;
    const int K = gm.Cin * tap2;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int mt = cdiv(gm.Cout, BM), pt = cdiv(P, BP);
    ConvPlan pl = {};
    pl.split = split_reduction(K, mt * pt * gm.G);
    pl.grid = dim3(mt, pt, gm.G * pl.split);
    const bool staged = !fp8 && (P % BP == 0 || P >= BP) && OHW % BP == 0
                        && BP % gm.OW == 0
                        && (gm.W + 2 * gm.pad) <= WIN_W - 2
                        && ((BP / gm.OW - 1) * gm.stride + gm.khw) <= WIN_ROWS
                        && (BK / tap2 + 2) <= WIN_CH;
    // resident window: wherever the staged kernel is routed and the slice's
    // window fits under the LDS cap
    const int nkc = cdiv(cdiv(K, BK), pl.split);
    int win_bytes = 0;
    if (staged && resident_on() && P % BP == 0 && 2 * gm.pad <= WGAP
        && resident_window_fits(nkc, tap2, gm.Cin,
                                (BP / gm.OW - 1) * gm.stride + gm.khw, gm.W,
                                esz, 2, &win_bytes)) {
        pl.route = RESIDENT;
        pl.tab0 = win_bytes;                     // ushort k-offset table
        pl.dyn_lds = win_bytes + nkc * BK * 2;
    } else if (staged) {
        pl.route = STAGED;
    } else {
        pl.route = GATHER;
        pl.fp8 = fp8 && esz == 2;
        // offsets cin*HW + kh*W + kw are packed above a 4-bit tap index
        pl.tabled = !fp8 && tabled_on() && gm.khw <= 3
                    && nkc * BK <= TAB_CAP
                    && (long)gm.Cin * gm.H * gm.W < (1L << 27);
        pl.tab_lds = nkc * BK * 4;
    }
    return pl;
}

static ConvPlan plan_bwd_data(const ConvGeom& gm, int esz, bool fp8) {
    const int tap2 = gm.khw * gm.khw;
    const int Q = gm.N * gm.H * gm.W;
    const bool s2 = (gm.stride == 2 && gm.H % 2 == 0 && gm.W % 2 == 0);
    // parity path: 4 classes of Q/4 pixels, ~1/4 the taps each
    const int Jfull = gm.Cout * tap2;
    const int J = s2 ? (Jfull + 3) / 4 : Jfull;
    const int ct = cdiv(gm.Cin, BM);
    ConvPlan pl = {};
    pl.nyp = cdiv(s2 ? Q / 4 : Q, BP);
    const int qt = pl.nyp * (s2 ? 4 : 1);
    pl.split = split_reduction(J, ct * qt * gm.G);
    pl.grid = dim3(ct, qt, gm.G * pl.split);
    const bool q = fp8 && esz == 2;
    const bool staged = !q && !s2 && gm.stride == 1
                        && (gm.H * gm.W) % BP == 0 && BP % gm.W == 0
                        && (gm.OW + 2 * gm.pad) <= WIN_W - 2
                        && (BP / gm.W + gm.khw - 1) <= WIN_ROWS
                        && (BK / tap2 + 2) <= WIN_CH;
    // resident dy window (2*pad >= khw-1: the geometry the staged kernel's
    // own window addressing covers)
    const int njc = cdiv(cdiv(J, BK), pl.split);
    int win_bytes = 0;
    if (staged && !fp8 && resident_on() && 2 * gm.pad <= WGAP
        && 2 * gm.pad >= gm.khw - 1
        && resident_window_fits(njc, tap2, gm.Cout, BP / gm.W + gm.khw - 1,
                                gm.OW, esz, 6, &win_bytes)) {
        pl.route = RESIDENT;
        pl.tab0 = win_bytes;                     // int weight-offset table
        pl.tab1 = win_bytes + njc * BK * 4;      // ushort window-offset table
        pl.dyn_lds = win_bytes + njc * BK * 6;
    } else if (staged) {
        pl.route = STAGED;
    } else {
        pl.route = s2 ? GATHER_S2 : GATHER;
        pl.fp8 = q;
        // the kernel's own slice: a parity class carries up to
        // ceil(khw/2)^2 taps per output channel
        const int t1 = s2 ? (gm.khw + 1) / 2 : gm.khw;
        const int nj = cdiv(cdiv(gm.Cout * t1 * t1, BK), pl.split);
        pl.tabled = !fp8 && tabled_on() && gm.khw <= 3
                    && nj * BK <= TAB_CAP
                    && (long)gm.Cout * gm.OH * gm.OW < (1L << 26)
                    && (long)gm.Cout * gm.Cin * tap2 < (1L << 31);
        pl.tab_lds = nj * BK * 8;
    }
    return pl;
}

static ConvPlan plan_bwd_weight(const ConvGeom& gm, int esz, bool fp8) {
    const int K = gm.Cin * gm.khw * gm.khw;
    const int OHW = gm.OH * gm.OW;
    const int P = gm.N * OHW;
    const int mt = cdiv(gm.Cout, BM), kt = cdiv(K, BP);
    const int mk_tiles = mt * kt * gm.G;
    ConvPlan pl = {};
    pl.split = 1;
    // measured (bwdw2 r2): small-P shapes that already have >=512 (m,k)
    // tiles need no split at all — L3 bwdW 89.4us (splitp 2) -> 74.5us
    // (splitp 1) = 1.00x MIOpen; splitting only pays when tiles are scarce
    // or P is long enough to amortize the partial reduce
    if (P > 1024 || mk_tiles < 512)
        while (mk_tiles * pl.split < split_target()
               && pl.split * BK * 4 < P)
            pl.split *= 2;
    pl.grid = dim3(mt, kt, gm.G * pl.split);
    const bool q = fp8 && esz == 2;
    // staged path: 3x3 kernels (a 64-wide k-tile then spans <= 9 input
    // channels = WWIN_CH), p-steps inside one sample spanning whole rows
    const bool staged = !q && gm.khw == 3 && OHW % BK == 0 && BK % gm.OW == 0
                        && (gm.W + 2 * gm.pad) <= WIN_W - 2
                        && ((BK / gm.OW - 1) * gm.stride + gm.khw) <= WIN_ROWS;
    if (!staged) {
        pl.route = GATHER;
        pl.fp8 = q;
        // int pixel bases: both tensors index below 2^31
        pl.tabled = !fp8 && tabled_on() && gm.khw <= 3
                    && cdiv(P, pl.split) <= PIX_TAB_CAP
                    && (long)gm.N * gm.G * gm.Cin * gm.H * gm.W < (1L << 31)
                    && (long)gm.N * gm.G * gm.Cout * OHW < (1L << 31);
        return pl;
    }
    // resident x window: one sample segment of the p-chunk at a time
    const int pchunk = cdiv(cdiv(P, pl.split), BK) * BK;
    const long wwin = (long)std::min(gm.Cin, WWIN_CH)
                          * ((std::min(pchunk, OHW) / gm.OW - 1) * gm.stride
                             + gm.khw) * (gm.W + WGAP) + WGAP;
    if (resident_on() && 2 * gm.pad <= WGAP
        && 2L * (BM + BP) * LDK * esz + wwin * esz <= resident_lds_cap()) {
        pl.route = RESIDENT;
        pl.dyn_lds = (int)((wwin * esz + 15) / 16 * 16);
    } else {
        pl.route = STAGED;
    }
    return pl;
}

std::tuple<std::string, int64_t, int64_t> conv_plan(
        const std::string& direction, int64_t G, int64_t N, int64_t Cin,
        int64_t H, int64_t W, int64_t Cout, int64_t khw, int64_t stride,
        int64_t pad, int64_t elem_size, int64_t fp8) {
    TORCH_CHECK(elem_size == 2 || elem_size == 4, "elem_size must be 2 or 4");
    const ConvGeom gm = conv_geom(G, N, Cin, H, W, Cout, khw, stride, pad);
    ConvPlan pl;
    if (direction == "fwd")
        pl = plan_fwd(gm, (int)elem_size, fp8 != 0);
    else if (direction == "bwd_data")
        pl = plan_bwd_data(gm, (int)elem_size, fp8 != 0);
    else if (direction == "bwd_weight")
        pl = plan_bwd_weight(gm, (int)elem_size, fp8 != 0);
    else
        TORCH_CHECK(false, "direction must be fwd, bwd_data or bwd_weight");
    static const char* const names[] = {"gather", "gather_s2", "staged",
                                        "resident"};
    return {std::string(names[pl.route]) + (pl.fp8 ? "_fp8" : ""), pl.split,
            pl.dyn_lds};
}

// Name of the kernel the launcher of `direction` would launch for this
// shape (template arguments left out; "<fp8>" marks the fp8 tile
// instantiation).  conv_plan()'s route string does not tell the tabled
// gather kernels from the untabled ones; this does.
std::string conv_plan_variant(
        const std::string& direction, int64_t G, int64_t N, int64_t Cin,
        int64_t H, int64_t W, int64_t Cout, int64_t khw, int64_t stride,
        int64_t pad, int64_t elem_size, int64_t fp8) {
    TORCH_CHECK(elem_size == 2 || elem_size == 4, "elem_size must be 2 or 4");
    const ConvGeom gm = conv_geom(G, N, Cin, H, W, Cout, khw, stride, pad);
    ConvPlan pl;
    std::string stem;
    if (direction == "fwd") {
        pl = plan_fwd(gm, (int)elem_size, fp8 != 0);
        stem = "conv_fwd";
    } else if (direction == "bwd_data") {
        pl = plan_bwd_data(gm, (int)elem_size, fp8 != 0);
        stem = pl.route == GATHER_S2 ? "conv_bwd_data_s2" : "conv_bwd_data";
    } else if (direction == "bwd_weight") {
        pl = plan_bwd_weight(gm, (int)elem_size, fp8 != 0);
        stem = "conv_bwd_weight";
    } else {
        TORCH_CHECK(false, "direction must be fwd, bwd_data or bwd_weight");
    }
    if (pl.route == RESIDENT) return stem + "_resident_kernel";
    if (pl.route == STAGED) return stem + "_staged_kernel";
    if (pl.tabled) return stem + "_tabled_kernel";
    return stem + (pl.fp8 ? "_kernel<fp8>" : "_kernel");
}

#define DISPATCH_CONV_FT(t, ...)                                              \
    if ((t) == at::kFloat) { using scalar_t = float; __VA_ARGS__; }           \
    else if ((t) == at::kBFloat16) { using scalar_t = __hip_bfloat16; __VA_ARGS__; } \
    else { TORCH_CHECK(false, "unsupported dtype"); }

// Split-K reduce of fwd / bwd-data: the float4 kernel when the tensor is a
// whole number of 4-element vectors at aligned bases, else (and with
// HETEROFL_STREAM_VEC=0) the one-float-per-lane kernel for the whole tensor.
template <typename T>
static void launch_out_reduce(hipStream_t stream, const float* pp,
                              const float* bp, const T* rp, T* yp, long total,
                              long chanstride, int nchan, int split) {
    const bool vec = stream_vec_on() && total % 4 == 0 &&
                     ptr_aligned(pp, 16) && ptr_aligned(yp, 4 * sizeof(T)) &&
                     (!rp || ptr_aligned(rp, 4 * sizeof(T)));
    if (!vec) {
        hipLaunchKernelGGL(conv_out_reduce_kernel<T>,
                           dim3((int)((total + 255) / 256)), dim3(256), 0,
                           stream, pp, bp, rp, yp, total, chanstride, nchan,
                           split);
        return;
    }
    const bool wide = total >= (1L << 31);
    auto kern = !bp ? conv_out_reduce_vec_kernel<T, 0, int>
                : chanstride % 4 == 0
                    ? (wide ? conv_out_reduce_vec_kernel<T, 1, long>
                            : conv_out_reduce_vec_kernel<T, 1, int>)
                    : (wide ? conv_out_reduce_vec_kernel<T, 2, long>
                            : conv_out_reduce_vec_kernel<T, 2, int>);
    hipLaunchKernelGGL(kern, dim3((int)((total / 4 + 255) / 256)), dim3(256),
                       0, stream, pp, bp, rp, yp, total, chanstride, nchan,
                       split);
}

// The non-resident kernels of a direction share a signature: pick by plan.
// fp8 tiles are instantiated for bf16 tensors only.
template <typename T>
static auto fwd_kernel(const ConvPlan& pl) {
    if (pl.route == STAGED) return conv_fwd_staged_kernel<T, T, T>;
    if constexpr (std::is_same<T, __hip_bfloat16>::value)
        if (pl.fp8) return conv_fwd_kernel<T, e4m3, e4m3>;
    return conv_fwd_kernel<T, T, T>;
}
template <typename T>
static auto bwd_data_kernel(const ConvPlan& pl) {
    if (pl.route == STAGED) return conv_bwd_data_staged_kernel<T, T, T>;
    if constexpr (std::is_same<T, __hip_bfloat16>::value)
        if (pl.fp8) return conv_bwd_data_kernel<T, e4m3, e5m2>;
    return conv_bwd_data_kernel<T, T, T>;
}
template <typename T>
static auto bwd_data_s2_kernel(const ConvPlan& pl) {
    if constexpr (std::is_same<T, __hip_bfloat16>::value)
        if (pl.fp8) return conv_bwd_data_s2_kernel<T, e4m3, e5m2>;
    return conv_bwd_data_s2_kernel<T, T, T>;
}
template <typename T>
static auto bwd_weight_kernel(const ConvPlan& pl) {
    if (pl.route == STAGED) return conv_bwd_weight_staged_kernel<T, T, T>;
    if constexpr (std::is_same<T, __hip_bfloat16>::value)
        if (pl.fp8) return conv_bwd_weight_kernel<T, e5m2, e4m3>;
    return conv_bwd_weight_kernel<T, T, T>;
}

at::Tensor conv_fwd(at::Tensor x, at::Tensor w, at::Tensor bias,
                    at::Tensor residual, int64_t groups, int64_t stride,
                    int64_t pad, int64_t fp8) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && w.is_contiguous());
    TORCH_CHECK(w.scalar_type() == at::kFloat, "weights must be fp32 master");
    const ConvGeom gm = conv_geom(groups, x.size(0), w.size(1), x.size(2),
                                  x.size(3), w.size(0) / groups, w.size(2),
                                  stride, pad);
    const int esz = (int)x.element_size();
    const ConvPlan pl = plan_fwd(gm, esz, fp8 != 0);
    auto y = at::empty({gm.N, gm.G * gm.Cout, gm.OH, gm.OW}, x.options());
    at::Tensor partial;
    if (pl.split > 1)
        partial = at::empty({(long)pl.split * y.numel()},
                            x.options().dtype(at::kFloat));
    float* pp = pl.split > 1 ? partial.data_ptr<float>() : nullptr;
    const float* wp = w.data_ptr<float>();
    const float* bp = bias.defined() ? bias.data_ptr<float>() : nullptr;
    auto stream = at::hip::getCurrentHIPStream();
    DISPATCH_CONV_FT(x.scalar_type(), {
        const scalar_t* xp = (const scalar_t*)x.data_ptr();
        const scalar_t* rp = residual.defined()
                                 ? (const scalar_t*)residual.data_ptr()
                                 : nullptr;
        scalar_t* yp = (scalar_t*)y.data_ptr();
        if (pl.route == RESIDENT) {
            const int K = gm.Cin * gm.khw * gm.khw;
            const int flags =
                ((gm.W % (16 / esz) == 0 && aligned16(xp)) ? 1 : 0)
                | ((K % 4 == 0 && aligned16(wp)) ? 2 : 0);
            hipLaunchKernelGGL(conv_fwd_resident_kernel<scalar_t>, pl.grid,
                               dim3(256), pl.dyn_lds, stream, xp, wp, bp, rp,
                               yp, pp, gm, pl.split, pl.tab0, flags);
        } else if (pl.tabled) {
            const int K = gm.Cin * gm.khw * gm.khw;
            const int flags = (K % 4 == 0 && aligned16(wp)) ? 2 : 0;
            hipLaunchKernelGGL(conv_fwd_tabled_kernel<scalar_t>, pl.grid,
                               dim3(256), pl.tab_lds, stream, xp, wp, bp, rp, yp, pp,
                               gm, pl.split, flags);
        } else {
            hipLaunchKernelGGL(fwd_kernel<scalar_t>(pl), pl.grid, dim3(256),
                               0, stream, xp, wp, bp, rp, yp, pp, gm,
                               pl.split);
        }
        if (pl.split > 1) {
            const long total = y.numel();
            launch_out_reduce<scalar_t>(stream, pp, bp, rp, yp, total,
                                        (long)gm.OH * gm.OW, gm.G * gm.Cout,
                                        pl.split);
        }
    });
    return y;
}

at::Tensor conv_bwd_data(at::Tensor dy, at::Tensor w, int64_t groups,
                         int64_t stride, int64_t pad, int64_t H, int64_t W,
                         int64_t fp8) {
    TORCH_CHECK(dy.is_cuda() && w.is_contiguous());
    TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2");
    auto dyc = dy.contiguous();
    const ConvGeom gm = conv_geom(groups, dy.size(0), w.size(1), H, W,
                                  w.size(0) / groups, w.size(2), stride, pad);
    TORCH_CHECK(dy.size(2) == gm.OH && dy.size(3) == gm.OW,
                "dy does not match the conv geometry");
    const int esz = (int)dy.element_size();
    const ConvPlan pl = plan_bwd_data(gm, esz, fp8 != 0);
    auto dx = at::empty({gm.N, gm.G * gm.Cin, gm.H, gm.W}, dy.options());
    at::Tensor partial;
    if (pl.split > 1)
        partial = at::empty({(long)pl.split * dx.numel()},
                            dy.options().dtype(at::kFloat));
    float* pp = pl.split > 1 ? partial.data_ptr<float>() : nullptr;
    const float* wp = w.data_ptr<float>();
    auto stream = at::hip::getCurrentHIPStream();
    DISPATCH_CONV_FT(dy.scalar_type(), {
        const scalar_t* dyp = (const scalar_t*)dyc.data_ptr();
        scalar_t* dxp = (scalar_t*)dx.data_ptr();
        if (pl.route == RESIDENT) {
            const int flags =
                (gm.OW % (16 / esz) == 0 && aligned16(dyp)) ? 1 : 0;
            hipLaunchKernelGGL(conv_bwd_data_resident_kernel<scalar_t>,
                               pl.grid, dim3(256), pl.dyn_lds, stream, dyp,
                               wp, dxp, pp, gm, pl.split, pl.tab0, pl.tab1,
                               flags);
        } else if (pl.tabled && pl.route == GATHER_S2) {
            hipLaunchKernelGGL(conv_bwd_data_s2_tabled_kernel<scalar_t>,
                               pl.grid, dim3(256), pl.tab_lds, stream, dyp, wp, dxp,
                               pp, gm, pl.split, pl.nyp);
        } else if (pl.tabled) {
            hipLaunchKernelGGL(conv_bwd_data_tabled_kernel<scalar_t>,
                               pl.grid, dim3(256), pl.tab_lds, stream, dyp, wp, dxp,
                               pp, gm, pl.split);
        } else if (pl.route == GATHER_S2) {
            hipLaunchKernelGGL(bwd_data_s2_kernel<scalar_t>(pl), pl.grid,
                               dim3(256), 0, stream, dyp, wp, dxp, pp, gm,
                               pl.split, pl.nyp);
        } else {
            hipLaunchKernelGGL(bwd_data_kernel<scalar_t>(pl), pl.grid,
                               dim3(256), 0, stream, dyp, wp, dxp, pp, gm,
                               pl.split);
        }
        if (pl.split > 1) {
            const long total = dx.numel();
            launch_out_reduce<scalar_t>(stream, pp, nullptr, nullptr, dxp,
                                        total, 1L, 1, pl.split);
        }
    });
    return dx;
}

at::Tensor conv_bwd_weight(at::Tensor dy, at::Tensor x, int64_t groups,
                           int64_t stride, int64_t pad, int64_t khw,
                           int64_t fp8) {
    auto dyc = dy.contiguous();
    const ConvGeom gm = conv_geom(groups, x.size(0), x.size(1) / groups,
                                  x.size(2), x.size(3), dy.size(1) / groups,
                                  khw, stride, pad);
    TORCH_CHECK(dy.size(2) == gm.OH && dy.size(3) == gm.OW,
                "dy does not match the conv geometry");
    const int esz = (int)x.element_size();
    const ConvPlan pl = plan_bwd_weight(gm, esz, fp8 != 0);
    const long GK = (long)gm.G * gm.Cout * gm.Cin * gm.khw * gm.khw;
    auto dw = at::empty({(long)gm.G * gm.Cout, gm.Cin, gm.khw, gm.khw},
                        x.options().dtype(at::kFloat));
    // split-P partials are summed in fixed order by splitp_reduce_kernel
    at::Tensor partials;
    if (pl.split > 1)
        partials = at::empty({pl.split, GK}, x.options().dtype(at::kFloat));
    float* out = pl.split > 1 ? partials.data_ptr<float>()
                              : dw.data_ptr<float>();
    auto stream = at::hip::getCurrentHIPStream();
    DISPATCH_CONV_FT(x.scalar_type(), {
        const scalar_t* dyp = (const scalar_t*)dyc.data_ptr();
        const scalar_t* xp = (const scalar_t*)x.data_ptr();
        if (pl.route == RESIDENT) {
            const int flags =
                ((gm.W % (16 / esz) == 0 && aligned16(xp)) ? 1 : 0)
                | (aligned16(dyp) ? 2 : 0);
            hipLaunchKernelGGL(conv_bwd_weight_resident_kernel<scalar_t>,
                               pl.grid, dim3(256), pl.dyn_lds, stream, dyp,
                               xp, out, gm, pl.split, flags);
        } else if (pl.tabled) {
            const int OHW = gm.OH * gm.OW;
            const int pchunk = cdiv(gm.N * OHW, pl.split);
            const int flags = (OHW % 8 == 0 && pchunk % 8 == 0
                               && aligned16(dyp)) ? 2 : 0;
            hipLaunchKernelGGL(conv_bwd_weight_tabled_kernel<scalar_t>,
                               pl.grid, dim3(256), 0, stream, dyp, xp, out,
                               gm, pl.split, flags);
        } else {
            hipLaunchKernelGGL(bwd_weight_kernel<scalar_t>(pl), pl.grid,
                               dim3(256), 0, stream, dyp, xp, out, gm,
                               pl.split);
        }
    });
    if (pl.split > 1) {
        if (stream_vec_on() && GK % 4 == 0 && aligned16(out) &&
            aligned16(dw.data_ptr<float>()))
            hipLaunchKernelGGL(splitp_reduce_vec_kernel,
                               dim3((int)((GK / 4 + 255) / 256)), dim3(256),
                               0, stream, out, dw.data_ptr<float>(), GK,
                               pl.split);
        else
            hipLaunchKernelGGL(splitp_reduce_kernel,
                               dim3((int)((GK + 255) / 256)), dim3(256), 0,
                               stream, out, dw.data_ptr<float>(), GK,
                               pl.split);
    }
    return dw;
}

// --------------------------------------------------- MFMA layout self-test
__global__ void mfma_probe_kernel(const float* __restrict__ A,
                                  const float* __restrict__ B,
                                  float* __restrict__ D) {
    const int l = threadIdx.x;
    const int kb = (l >> 4) * 8;
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = (__bf16)A[(l & 15) * 32 + kb + j];
        b[j] = (__bf16)B[(kb + j) * 16 + (l & 15)];
    }
    f32x4 acc = {};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        D[((l >> 4) * 4 + r) * 16 + (l & 15)] = acc[r];
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
    TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
                B.sizes() == at::IntArrayRef({32, 16}));
    auto Ac = A.contiguous().to(at::kFloat).cuda();
    auto Bc = B.contiguous().to(at::kFloat).cuda();
    auto D = at::empty({16, 16}, Ac.options());
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
                       Ac.data_ptr<float>(), Bc.data_ptr<float>(),
                       D.data_ptr<float>());
    return D;
}
