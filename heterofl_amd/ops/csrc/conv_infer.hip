// Large-batch forward-only convolution for inference and the sBN statistics
// pass (groups = 1, bf16 NCHW activations, fp32 MFMA accumulation).
//
// The training conv family (conv_mfma.hip) is tuned for batch 10: a 64x64
// tile, fp32 master weights re-read and converted on every K-step, and a
// per-element bounds-tested activation gather.  At statistics / evaluation
// batch sizes P = N*OH*OW is large and the weights are constant over a whole
// pass, so this kernel
//   - reads weights from a one-time bf16 repack (conv_pack_weight): K is
//     ordered tap-major, (kh, kw) outer and cin inner, with cin zero-padded
//     to a multiple of BK and Cout zero-padded to a multiple of 128.  A
//     BK=32 K-slab then lies inside one filter tap, so the border decision
//     is made once per (pixel, tap) and the A tile is plain 16-byte loads
//     with no bounds tests;
//   - uses a 128 (M) x 128 (P) output tile, or 64 x 256 when Cout <= 64,
//     with each of the 4 waves owning a 64x64 sub-tile: one K-step issues
//     16 MFMAs against 8 16-byte fragment reads;
//   - loads the B tile with the pixel axis across lanes (coalesced along
//     NCHW's innermost axis); each thread owns one pixel and BK*BP/256
//     consecutive cin, and stores them k-contiguous ("transposed") into LDS
//     so the fragment reads are the same 16-byte [row][k] reads as in
//     conv_mfma.hip;
//   - double-buffers LDS with the next slab's global loads in flight under
//     the MFMAs (one barrier per K-step).
// No atomics and no split-K: every output element is produced by exactly one
// lane in a fixed summation order.
//
// Fragment layout of mfma_f32_16x16x32_bf16 (tests/test_gpu.py::
// test_mfma_probe_layout): A: lane l holds A[row=l%16][k=(l/16)*8+j];
// B: B[k=(l/16)*8+j][col=l%16]; C/D: row=(l/16)*4+reg, col=l%16.
#include "common.h"

namespace {

typedef unsigned short u16;

constexpr int LBK = 32;          // K-slab
constexpr int LLDK = LBK + 8;    // padded k-stride of the [row][k] LDS tiles
constexpr int MPAD = 128;        // Cout padding of the packed weight

struct LargeGeom {
    int N, H, W, Cin, Cout, OH, OW, khw, stride, pad;
    int Cinp;   // Cin rounded up to LBK
    int Kp;     // khw*khw*Cinp (row stride of the packed weight)
};

__global__ void __launch_bounds__(256)
conv_pack_weight_kernel(const float* __restrict__ w, u16* __restrict__ out,
                        int Cout, int Cin, int kk2, int Cinp, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int Kp = kk2 * Cinp;
    const int m = (int)(i / Kp);
    const int r = (int)(i - (long)m * Kp);
    const int tap = r / Cinp, c = r - tap * Cinp;
    float v = 0.f;
    if (m < Cout && c < Cin) v = w[((long)m * Cin + c) * kk2 + tap];
    __hip_bfloat16 b = __float2bfloat16(v);
    out[i] = *reinterpret_cast<u16*>(&b);
}

__device__ __forceinline__ float bf16_bits_to_f32(u16 v) {
    return __uint_as_float((unsigned)v << 16);
}
__device__ __forceinline__ u16 f32_to_bf16_bits(float v) {
    __hip_bfloat16 b = __float2bfloat16(v);
    return *reinterpret_cast<u16*>(&b);
}

// grid: 1-D, m-tile fastest (blocks that share a B tile run back to back).
template <int TBM, int TBP>
__global__ void __launch_bounds__(256)
conv_fwd_large_kernel(const u16* __restrict__ x, const u16* __restrict__ wp,
                      const float* __restrict__ bias,
                      const u16* __restrict__ residual, u16* __restrict__ y,
                      LargeGeom gm, int mtiles) {
    constexpr int WPN = TBP / 64;            // waves along P
    constexpr int TPP = 256 / TBP;           // threads per pixel (2 or 1)
    constexpr int KPT = LBK / TPP;           // cin per thread per slab
    constexpr int AV = TBM * LBK / 8 / 256;  // 16-byte A loads per thread
    static_assert(TBM * TBP == 128 * 128, "4 waves x 64x64");
    static_assert(TPP * TBP == 256 && AV >= 1, "loader mapping");
    __shared__ u16 a_lds[2][TBM][LLDK];
    __shared__ u16 b_lds[2][TBP][LLDK];
    __shared__ long t_ybase[TBP];

    const int mt = blockIdx.x % mtiles;
    const int pt = blockIdx.x / mtiles;
    const int m0 = mt * TBM;
    const long p0 = (long)pt * TBP;
    const int OHW = gm.OH * gm.OW;
    const long P = (long)gm.N * OHW;
    const long HW = (long)gm.H * gm.W;
    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int wm = (wave / WPN) * 64;
    const int wpx = (wave % WPN) * 64;

    // this thread's loader pixel (fixed for the whole K loop)
    const int lp = tid % TBP;
    // first cin of this thread inside a slab: the same for a whole wave
    const int lk = __builtin_amdgcn_readfirstlane((tid / TBP) * KPT);
    int ihb, iwb;
    long xbase;
    {
        const long p = p0 + lp;
        if (p < P) {
            const int n = (int)(p / OHW);
            const int hw = (int)(p - (long)n * OHW);
            const int oh = hw / gm.OW, ow = hw - oh * gm.OW;
            ihb = oh * gm.stride - gm.pad;
            iwb = ow * gm.stride - gm.pad;
            xbase = (long)n * gm.Cin * HW;
            if (tid < TBP) t_ybase[lp] = (long)n * gm.Cout * OHW + hw;
        } else {
            ihb = -(1 << 28);  // every tap lands out of bounds -> zeros
            iwb = -(1 << 28);
            xbase = 0;
            if (tid < TBP) t_ybase[lp] = -1;
        }
    }

    const int cpt = gm.Cinp / LBK;          // slabs per tap
    const int nsteps = gm.khw * gm.khw * cpt;

    u16x8 ra[AV];
    u16 rb[KPT];
    // loader state for the NEXT slab to fetch: (kh, kw, c0); r_inb / r_c0
    // describe the slab currently held in rb
    int s_kh = 0, s_kw = 0, s_c0 = 0, s_idx = 0;
    bool r_inb = false;
    int r_c0 = 0;
    auto load_regs = [&]() {
        // A: packed rows are padded to MPAD and Kp, no bounds tests
        const int kcol = s_idx * LBK + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int row = m0 + (tid >> 2) + i * 64;
            ra[i] = *(const u16x8*)(wp + (long)row * gm.Kp + kcol);
        }
        // B: one border decision for this (pixel, tap).  The loads are
        // unconditional so that all KPT of them are in flight together
        // (predicated loads serialise on memory latency): a pixel outside
        // the image reads offset 0 and a padded cin reads channel Cin-1,
        // both inside x; store_lds zeroes those values.  The channel offset
        // is wave-uniform, so it stays in scalar registers.
        const int ih = ihb + s_kh, iw = iwb + s_kw;
        r_inb = ih >= 0 && ih < gm.H && iw >= 0 && iw < gm.W;
        r_c0 = s_c0 + lk;
        const u16* src = x + (r_inb ? xbase + (long)ih * gm.W + iw : 0L);
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            rb[j] = src[(long)min(r_c0 + j, gm.Cin - 1) * HW];
        // advance to the following slab
        ++s_idx;
        s_c0 += LBK;
        if (s_c0 == gm.Cinp) {
            s_c0 = 0;
            if (++s_kw == gm.khw) { s_kw = 0; ++s_kh; }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AV; ++i)
            *(u16x8*)&a_lds[buf][(tid >> 2) + i * 64][(tid & 3) * 8] = ra[i];
#pragma unroll
        for (int q = 0; q < KPT / 8; ++q) {
            u16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // AND with a mask, not a select: a select lets the compiler
                // sink the load back under a branch
                const u16 keep = (r_inb && r_c0 + q * 8 + j < gm.Cin)
                                     ? (u16)0xFFFF : (u16)0;
                v[j] = rb[q * 8 + j] & keep;
            }
            *(u16x8*)&b_lds[buf][lp][lk + q * 8] = v;
        }
    };

    f32x4 acc[4][4] = {};
    load_regs();
    store_lds(0);
    if (nsteps > 1) load_regs();
    __syncthreads();
    int cur = 0;
    const int kb = (l >> 4) * 8;
    for (int s = 0; s < nsteps; ++s) {
        bf16x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = *(const bf16x8*)&a_lds[cur][wm + i * 16 + (l & 15)][kb];
            fb[i] = *(const bf16x8*)&b_lds[cur][wpx + i * 16 + (l & 15)][kb];
        }
#pragma unroll
        for (int fm = 0; fm < 4; ++fm)
#pragma unroll
            for (int fp = 0; fp < 4; ++fp)
                acc[fm][fp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    fa[fm], fb[fp], acc[fm][fp], 0, 0, 0);
        if (s + 1 < nsteps) {
            store_lds(cur ^ 1);
            if (s + 2 < nsteps) load_regs();
        }
        __syncthreads();
        cur ^= 1;
    }

    // epilogue: bias, residual add, bf16 round; lanes run along the pixel axis
#pragma unroll
    for (int fp = 0; fp < 4; ++fp) {
        const long yb = t_ybase[wpx + fp * 16 + (l & 15)];
        if (yb < 0) continue;
#pragma unroll
        for (int fm = 0; fm < 4; ++fm) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + fm * 16 + (l >> 4) * 4 + r;
                if (m < gm.Cout) {
                    const long off = yb + (long)m * OHW;
                    float v = acc[fm][fp][r];
                    if (bias) v += bias[m];
                    if (residual) v += bf16_bits_to_f32(residual[off]);
                    y[off] = f32_to_bf16_bits(v);
                }
            }
        }
    }
}

}  // namespace

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

at::Tensor conv_pack_weight(at::Tensor w) {
    TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.size(2) == w.size(3),
                "conv_pack_weight: (Cout, Cin, k, k) device tensor expected");
    auto wc = w.contiguous().to(at::kFloat);
    const int Cout = wc.size(0), Cin = wc.size(1), k = wc.size(2);
    const int Cinp = round_up(Cin, LBK), Mp = round_up(Cout, MPAD);
    const long total = (long)Mp * k * k * Cinp;
    auto out = at::empty({Mp, (long)k * k * Cinp},
                         wc.options().dtype(at::kBFloat16));
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(conv_pack_weight_kernel,
                       dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       stream, wc.data_ptr<float>(), (u16*)out.data_ptr(),
                       Cout, Cin, k * k, Cinp, total);
    return out;
}

at::Tensor conv_fwd_large(at::Tensor x, at::Tensor packed, at::Tensor bias,
                          at::Tensor residual, int64_t stride, int64_t pad,
                          int64_t Cin, int64_t Cout, int64_t k) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4
                && x.scalar_type() == at::kBFloat16,
                "conv_fwd_large: contiguous bf16 NCHW input expected");
    TORCH_CHECK(x.size(1) == Cin, "conv_fwd_large: input channels != Cin");
    TORCH_CHECK((k == 3 && pad == 1) || (k == 1 && pad == 0),
                "conv_fwd_large: 3x3/pad 1 or 1x1/pad 0 only");
    TORCH_CHECK(stride == 1 || stride == 2, "conv_fwd_large: stride 1 or 2");
    TORCH_CHECK(Cin >= 1 && Cout >= 1 && x.size(0) >= 1);
    LargeGeom gm;
    gm.N = x.size(0);
    gm.H = x.size(2);
    gm.W = x.size(3);
    gm.Cin = (int)Cin;
    gm.Cout = (int)Cout;
    gm.khw = (int)k;
    gm.stride = (int)stride;
    gm.pad = (int)pad;
    gm.OH = (gm.H + 2 * gm.pad - gm.khw) / gm.stride + 1;
    gm.OW = (gm.W + 2 * gm.pad - gm.khw) / gm.stride + 1;
    gm.Cinp = round_up(gm.Cin, LBK);
    gm.Kp = gm.khw * gm.khw * gm.Cinp;
    const int Mp = round_up(gm.Cout, MPAD);
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous()
                && packed.scalar_type() == at::kBFloat16
                && packed.numel() == (long)Mp * gm.Kp,
                "conv_fwd_large: weight was not packed for this shape");
    TORCH_CHECK(gm.OH >= 1 && gm.OW >= 1);
    auto y = at::empty({gm.N, gm.Cout, gm.OH, gm.OW}, x.options());
    // an empty tensor stands for "absent", as in the other ops
    const bool has_bias = bias.defined() && bias.numel() > 0;
    const bool has_res = residual.defined() && residual.numel() > 0;
    if (has_bias)
        TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.is_contiguous()
                    && bias.numel() == Cout);
    if (has_res)
        TORCH_CHECK(residual.scalar_type() == at::kBFloat16
                    && residual.is_contiguous()
                    && residual.sizes() == y.sizes());
    const long P = (long)gm.N * gm.OH * gm.OW;
    auto stream = at::hip::getCurrentHIPStream();
    const float* bp = has_bias ? bias.data_ptr<float>() : nullptr;
    const u16* rp = has_res ? (const u16*)residual.data_ptr()
                                       : nullptr;
    if (gm.Cout <= 64) {
        const int mtiles = 1;
        const long ptiles = (P + 255) / 256;
        TORCH_CHECK(ptiles * mtiles < (1L << 31));
        hipLaunchKernelGGL((conv_fwd_large_kernel<64, 256>),
                           dim3((unsigned)(ptiles * mtiles)), dim3(256), 0,
                           stream, (const u16*)x.data_ptr(),
                           (const u16*)packed.data_ptr(), bp, rp,
                           (u16*)y.data_ptr(), gm, mtiles);
    } else {
        const int mtiles = (gm.Cout + 127) / 128;
        const long ptiles = (P + 127) / 128;
        TORCH_CHECK(ptiles * mtiles < (1L << 31));
        hipLaunchKernelGGL((conv_fwd_large_kernel<128, 128>),
                           dim3((unsigned)(ptiles * mtiles)), dim3(256), 0,
                           stream, (const u16*)x.data_ptr(),
                           (const u16*)packed.data_ptr(), bp, rp,
                           (u16*)y.data_ptr(), gm, mtiles);
    }
    return y;
}
