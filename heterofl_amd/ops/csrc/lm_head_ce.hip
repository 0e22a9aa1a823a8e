// Vocabulary projection fused with cross-entropy for masked-LM evaluation:
// row_lse[i] = logsumexp_j(x_i . W_j + b_j), row_nll[i] = row_lse[i] -
// logit[i, label_i], with the (M, V) logits never written to memory and never
// rounded to bf16.
//
//   - W comes from a one-time bf16 repack (lm_head_pack): (Vp, Ep) row-major
//     with E zero-padded to a multiple of the MFMA K (32) and V zero-padded to
//     a multiple of the 64-column tile, so the tile loads are plain 16-byte
//     loads with no bounds tests.
//   - A block owns 128 rows (4 waves x 32 rows).  Each lane loads its A
//     fragments of x for the whole K extent (E <= 256) into registers once;
//     they stay there for the whole vocabulary loop, so LDS holds only the
//     double-buffered 64-column W tile (2 x 64 x (KP+8) bf16: 66 KiB at
//     KP = 256, two blocks per CU).
//   - Per column tile a wave runs KP/32 k-steps of 2x4 mfma_f32_16x16x32_bf16
//     into fp32 accumulators, then folds the 32x64 logits into a per-lane
//     online (max, sum-exp) state.  A lane owns the columns congruent to
//     lane%16 of its 8 rows, so the vocabulary loop needs no cross-lane
//     traffic; the 16 lanes of a row are merged once at the end.
//   - vocab_mask follows lm_ce.hip / models/functional.py: a masked column's
//     logit is exactly 0 (bias included) and still takes part in the softmax.
//     Padded columns j >= V are given the logit -inf and take no part.
//   - The vocabulary is cut into `splits` contiguous runs of column tiles
//     (grid.y).  Every split writes its per-row (max, sum-exp) to a workspace
//     and a second kernel merges the splits in index order.  The label's
//     logit is written by the one lane that owns that column.  No atomics:
//     for a given `splits` the result is bit-reproducible.
//
// Fragment layout of mfma_f32_16x16x32_bf16: see conv_infer.hip.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef unsigned short u16;

constexpr int HBM = 128;   // rows per block
constexpr int HBN = 64;    // columns per tile (V padding of the packed weight)
constexpr int HBK = 32;    // MFMA K (E padding of the packed weight)
constexpr float NEG_BIG = -1e30f;

__global__ void __launch_bounds__(256)
lm_head_pack_kernel(const float* __restrict__ w, u16* __restrict__ out,
                    int V, int E, int Ep, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i / Ep);
    const int k = (int)(i - (long)j * Ep);
    float v = 0.f;
    if (j < V && k < E) v = w[(long)j * E + k];
    __hip_bfloat16 b = __float2bfloat16(v);
    out[i] = *reinterpret_cast<u16*>(&b);
}

// grid: (row tiles, splits).  KP: compile-time K capacity (>= Ep), it sizes
// the LDS tile and the register-resident x fragments.
template <int KP>
__global__ void __launch_bounds__(256, 2)
lm_head_ce_kernel(const u16* __restrict__ x, const u16* __restrict__ wp,
                  const float* __restrict__ bias,
                  const float* __restrict__ vmask,
                  const long* __restrict__ labels,
                  float* __restrict__ part_m, float* __restrict__ part_s,
                  float* __restrict__ lab_logit, int M, int E, int Ep, int V,
                  int ntiles) {
    constexpr int KS = KP / HBK;          // k-steps
    constexpr int LDK = KP + 8;           // padded k-stride of the LDS tile
    constexpr int CPR = KP / 8;           // 16-byte chunks per W row
    constexpr int NLD = HBN * CPR / 256;  // chunks per thread per tile
    static_assert(NLD >= 1 && NLD * 256 == HBN * CPR, "loader mapping");
    __shared__ u16 w_lds[2][HBN][LDK];

    const int tid = threadIdx.x;
    const int l = tid & (WAVE - 1);
    const int wave = tid / WAVE;
    const int splits = gridDim.y;
    const int sp = blockIdx.y;
    const int t0 = (int)((long)sp * ntiles / splits);
    const int t1 = (int)((long)(sp + 1) * ntiles / splits);
    const int row_base = blockIdx.x * HBM + wave * 32;
    const int lc = l & 15;   // fragment row (A/B operand) and C column
    const int lg = l >> 4;   // k group (operands) and C row group

    // x fragments for the whole K extent, zero beyond (M, E)
    bf16x8 xa[2][KS];
    const bool vec = (E & 7) == 0;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        const int row = row_base + fm * 16 + lc;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = ks * HBK + lg * 8;
            u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (row < M) {
                const u16* src = x + (long)row * E + k;
                if (vec && k + 8 <= E) {
                    v = *(const u16x8*)src;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (k + j < E) v[j] = src[j];
                }
            }
            xa[fm][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }

    // per-lane state of rows row_base + fm*16 + lg*4 + r
    float sm[2][4], ss[2][4], labv[2][4];
    int lab[2][4];
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row_base + fm * 16 + lg * 4 + r;
            sm[fm][r] = NEG_BIG;
            ss[fm][r] = 0.f;
            labv[fm][r] = 0.f;
            lab[fm][r] = row < M ? (int)labels[row] : -1;
        }

    // W loader: chunk c of a tile is row c / CPR, k (c % CPR) * 8.  The load
    // is unconditional (a chunk beyond Ep re-reads the row's last chunk) and
    // store_lds zeroes it.
    u16x8 rw[NLD];
    auto load_regs = [&](int t) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + i * 256;
            const int r = c / CPR, kc = (c % CPR) * 8;
            rw[i] = *(const u16x8*)(wp + ((long)t * HBN + r) * Ep
                                    + min(kc, Ep - 8));
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + i * 256;
            const int r = c / CPR, kc = (c % CPR) * 8;
            const u16 keep = kc < Ep ? (u16)0xFFFF : (u16)0;
            u16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = rw[i][j] & keep;
            *(u16x8*)&w_lds[buf][r][kc] = v;
        }
    };

    if (t0 < t1) {
        load_regs(t0);
        store_lds(0);
        if (t0 + 1 < t1) load_regs(t0 + 1);
    }
    __syncthreads();
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        // this tile's bias / mask values (column clamped into the vocabulary)
        float cb[4], ck[4];
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
            const int cc = min(t * HBN + fn * 16 + lc, V - 1);
            cb[fn] = bias ? bias[cc] : 0.f;
            ck[fn] = vmask ? vmask[cc] : 1.f;
        }
        f32x4 acc[2][4] = {};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 fb[4];
#pragma unroll
            for (int fn = 0; fn < 4; ++fn)
                fb[fn] = *(const bf16x8*)
                    &w_lds[cur][fn * 16 + lc][ks * HBK + lg * 8];
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 4; ++fn)
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        xa[fm][ks], fb[fn], acc[fm][fn], 0, 0, 0);
        }
        // next tile: registers -> the other buffer (last read before the
        // previous barrier), then start the loads of the tile after it
        if (t + 1 < t1) {
            store_lds(cur ^ 1);
            if (t + 2 < t1) load_regs(t + 2);
        }
        // fold the 32x64 logits into the online state
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v[4];
                float tmax = NEG_BIG;
#pragma unroll
                for (int fn = 0; fn < 4; ++fn) {
                    const int col = t * HBN + fn * 16 + lc;
                    float z = acc[fm][fn][r] + cb[fn];
                    z = ck[fn] != 0.f ? z : 0.f;
                    labv[fm][r] = col == lab[fm][r] ? z : labv[fm][r];
                    z = col < V ? z : -INFINITY;
                    v[fn] = z;
                    tmax = fmaxf(tmax, z);
                }
                const float mn = fmaxf(sm[fm][r], tmax);
                float s = ss[fm][r] * __expf(sm[fm][r] - mn);
#pragma unroll
                for (int fn = 0; fn < 4; ++fn) s += __expf(v[fn] - mn);
                sm[fm][r] = mn;
                ss[fm][r] = s;
            }
        __syncthreads();
        cur ^= 1;
    }

    // merge the 16 lanes of a row (fixed butterfly order), write the partial
    const int c0 = t0 * HBN;
    const int c1 = min(t1 * HBN, V);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = sm[fm][r], s = ss[fm][r];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const float mo = __shfl_xor(m, off, WAVE);
                const float so = __shfl_xor(s, off, WAVE);
                const float mn = fmaxf(m, mo);
                s = s * __expf(m - mn) + so * __expf(mo - mn);
                m = mn;
            }
            const int row = row_base + fm * 16 + lg * 4 + r;
            if (row < M) {
                if (lc == 0) {
                    part_m[(long)sp * M + row] = m;
                    part_s[(long)sp * M + row] = s;
                }
                const int y = lab[fm][r];
                if (y >= c0 && y < c1 && (y & 15) == lc)
                    lab_logit[row] = labv[fm][r];
            }
        }
}

__global__ void __launch_bounds__(256)
lm_head_merge_kernel(const float* __restrict__ part_m,
                     const float* __restrict__ part_s,
                     const float* __restrict__ lab_logit,
                     float* __restrict__ row_nll, float* __restrict__ row_lse,
                     int M, int splits) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    float m = NEG_BIG;
    for (int k = 0; k < splits; ++k) m = fmaxf(m, part_m[(long)k * M + row]);
    float s = 0.f;
    for (int k = 0; k < splits; ++k)
        s += part_s[(long)k * M + row]
             * __expf(part_m[(long)k * M + row] - m);
    const float lse = m + __logf(s);
    row_lse[row] = lse;
    row_nll[row] = lse - lab_logit[row];
}

}  // namespace

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

at::Tensor lm_head_pack(at::Tensor w) {
    TORCH_CHECK(w.is_cuda() && w.dim() == 2,
                "lm_head_pack: (V, E) device tensor expected");
    auto wc = w.contiguous().to(at::kFloat);
    const int V = wc.size(0), E = wc.size(1);
    TORCH_CHECK(V >= 1 && E >= 1 && E <= 256, "lm_head_pack: 1 <= E <= 256");
    const int Ep = round_up(E, HBK), Vp = round_up(V, HBN);
    const long total = (long)Vp * Ep;
    auto out = at::empty({Vp, Ep}, wc.options().dtype(at::kBFloat16));
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(lm_head_pack_kernel,
                       dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       stream, wc.data_ptr<float>(), (u16*)out.data_ptr(), V,
                       E, Ep, total);
    return out;
}

std::vector<at::Tensor> lm_head_ce(at::Tensor x, at::Tensor packed,
                                   at::Tensor bias, at::Tensor labels,
                                   at::Tensor vocab_mask, int64_t V,
                                   int64_t E, int64_t splits) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2
                && x.scalar_type() == at::kBFloat16,
                "lm_head_ce: contiguous bf16 (M, E) input expected");
    TORCH_CHECK(E >= 1 && E <= 256 && x.size(1) == E && V >= 1,
                "lm_head_ce: 1 <= E <= 256");
    const long Ml = x.size(0);
    TORCH_CHECK(Ml >= 1 && Ml < (1L << 31) - HBM, "lm_head_ce: bad M");
    const int M = (int)Ml;
    const int Ep = round_up((int)E, HBK), Vp = round_up((int)V, HBN);
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous()
                && packed.scalar_type() == at::kBFloat16
                && packed.numel() == (long)Vp * Ep,
                "lm_head_ce: weight was not packed for this shape");
    TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                && labels.scalar_type() == at::kLong && labels.numel() == M,
                "lm_head_ce: (M,) int64 labels expected");
    // an empty tensor stands for "absent", as in the other ops
    const bool has_bias = bias.defined() && bias.numel() > 0;
    const bool has_mask = vocab_mask.defined() && vocab_mask.numel() > 0;
    if (has_bias)
        TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat
                    && bias.is_contiguous() && bias.numel() == V);
    if (has_mask)
        TORCH_CHECK(vocab_mask.is_cuda()
                    && vocab_mask.scalar_type() == at::kFloat
                    && vocab_mask.is_contiguous() && vocab_mask.numel() == V);
    const int ntiles = Vp / HBN;
    const int rtiles = (M + HBM - 1) / HBM;
    if (splits <= 0) {
        // about two blocks per CU, but no split shorter than 10 column
        // tiles: below that the per-block prologue (x fragments) and the
        // merge outweigh the extra parallelism (splits sweep in
        // profiles/lm_inferbench.txt)
        const int cus = at::cuda::getCurrentDeviceProperties()
                            ->multiProcessorCount;
        splits = std::min((2 * cus + rtiles - 1) / rtiles,
                          std::max(ntiles / 10, 1));
    }
    if (splits > ntiles) splits = ntiles;
    TORCH_CHECK(splits >= 1 && splits <= 65535);
    auto opts = x.options().dtype(at::kFloat);
    auto part = at::empty({2, (long)splits, Ml}, opts);
    auto lab_logit = at::empty({Ml}, opts);
    auto row_nll = at::empty({Ml}, opts);
    auto row_lse = at::empty({Ml}, opts);
    float* pm = part.data_ptr<float>();
    float* ps = pm + (long)splits * Ml;
    auto stream = at::hip::getCurrentHIPStream();
    const float* bp = has_bias ? bias.data_ptr<float>() : nullptr;
    const float* mp = has_mask ? vocab_mask.data_ptr<float>() : nullptr;
    const dim3 grid((unsigned)rtiles, (unsigned)splits);
#define LAUNCH_HEAD(KP)                                                       \
    hipLaunchKernelGGL((lm_head_ce_kernel<KP>), grid, dim3(256), 0, stream,   \
                       (const u16*)x.data_ptr(),                              \
                       (const u16*)packed.data_ptr(), bp, mp,                 \
                       labels.data_ptr<long>(), pm, ps,                       \
                       lab_logit.data_ptr<float>(), M, (int)E, Ep, (int)V,    \
                       ntiles)
    if (Ep <= 32) LAUNCH_HEAD(32);
    else if (Ep <= 64) LAUNCH_HEAD(64);
    else if (Ep <= 128) LAUNCH_HEAD(128);
    else LAUNCH_HEAD(256);
#undef LAUNCH_HEAD
    hipLaunchKernelGGL(lm_head_merge_kernel, dim3((unsigned)((M + 255) / 256)),
                       dim3(256), 0, stream, pm, ps,
                       lab_logit.data_ptr<float>(),
                       row_nll.data_ptr<float>(), row_lse.data_ptr<float>(),
                       M, (int)splits);
    return {row_nll, row_lse};
}
