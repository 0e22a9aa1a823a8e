// Vocabulary projection fused with top-k for masked-LM fill-mask: the k
// largest logits of every row and their columns, next to the row's
// log-sum-exp and (optionally) the label's NLL, in one pass over the
// vocabulary.  Sibling of lm_head_ce.hip: the (M, V) logits never reach
// memory and are never rounded to bf16.
//
//   - The packed weight (lm_head_pack), the register-resident x fragments,
//     the double-buffered 64-column W tile, the MFMA mainloop and the online
//     (max, sum-exp) fold are those of lm_head_ce_kernel.  They are copied,
//     not shared: lm_head_ce's results have to stay bit-identical, and a
//     mainloop templated on its epilogue would let this kernel's register
//     pressure reshape that one's schedule.
//   - A lane owns the columns congruent to lane%16 of its 8 rows and meets
//     them in ascending order.  It keeps, per row, a list of the KC best
//     (value, column) pairs in registers, sorted by value descending and, for
//     equal values, column ascending.  A new logit is tested against the
//     list's last value only (strict >, so an equal later column never
//     displaces an earlier one); the insertion itself is a branch that is
//     rarely taken once the list has warmed up.
//   - After the loop the 16 lanes of a row are merged by k rounds of a
//     16-lane arg-max over the list heads ((value desc, column asc) is a
//     total order, so every lane sees the same winner); the winning lane pops
//     its head.  Lane 0 of the group writes the split's k candidates.
//   - Splits as in lm_head_ce: every split writes per-row (max, sum-exp) and
//     its own k candidates; a second kernel merges the splits.  No atomics:
//     for a given `splits` all outputs are bit-reproducible.
//   - A vocab-masked column's logit is exactly 0 and takes part in both the
//     softmax and the top-k.  Padded columns j >= V carry -inf, which never
//     beats a list entry, so they can not be returned.  Unfilled list slots
//     hold (-inf, INT_MAX); they sort behind every finite logit (logits are
//     assumed finite).
//
// Fragment layout of mfma_f32_16x16x32_bf16: see conv_infer.hip.
#include "common.h"

#include <climits>

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef unsigned short u16;

constexpr int HBM = 128;   // rows per block
constexpr int HBN = 64;    // columns per tile (V padding of the packed weight)
constexpr int HBK = 32;    // MFMA K (E padding of the packed weight)
constexpr float NEG_BIG = -1e30f;
constexpr int NO_COL = INT_MAX;   // column of an unfilled list slot
constexpr int MAX_K = 8;

// (va, ia) comes before (vb, ib): larger value, then lower column
__device__ __forceinline__ bool before(float va, int ia, float vb, int ib) {
    return va > vb || (va == vb && ia < ib);
}

// Blocks per CU asked of the compiler.  At KP = 256 the mainloop alone takes
// 238 registers (lm_head_ce_kernel<256>), so with 8 rows x KC (value,
// column) pairs on top two blocks per CU (256 registers) spill into scratch
// inside the vocabulary loop.  Measured at M = 32768, E = 256 (profiles/
// lm_inferbench.txt, "blocks per CU"): one block per CU (512 registers, no
// scratch) is 1.4x faster at KC = 5 and 2.4x at KC = 8, and 1.4x slower at
// KC = 1, whose spill is 28 bytes; KP = 64 is faster with two blocks at
// every KC.  KC = 3 at KP = 256 and all of KP = 128 were not measured and
// keep two blocks.
constexpr int min_blocks(int KP, int KC) {
    return KP == 256 && KC >= 5 ? 1 : 2;
}

// grid: (row tiles, splits).  KP: compile-time K capacity (>= Ep).  KC:
// capacity of the per-lane lists (>= k).
template <int KP, int KC>
__global__ void __launch_bounds__(256, min_blocks(KP, KC))
lm_head_topk_kernel(const u16* __restrict__ x, const u16* __restrict__ wp,
                    const float* __restrict__ bias,
                    const float* __restrict__ vmask,
                    const long* __restrict__ labels,
                    float* __restrict__ part_m, float* __restrict__ part_s,
                    float* __restrict__ cand_v, int* __restrict__ cand_i,
                    float* __restrict__ lab_logit, int M, int E, int Ep, int V,
                    int ntiles, int k) {
    constexpr int KS = KP / HBK;          // k-steps
    constexpr int LDK = KP + 8;           // padded k-stride of the LDS tile
    constexpr int CPR = KP / 8;           // 16-byte chunks per W row
    constexpr int NLD = HBN * CPR / 256;  // chunks per thread per tile
    static_assert(NLD >= 1 && NLD * 256 == HBN * CPR, "loader mapping");
    static_assert(KC >= 1 && KC <= MAX_K, "list capacity");
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
            const int kk = ks * HBK + lg * 8;
            u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (row < M) {
                const u16* src = x + (long)row * E + kk;
                if (vec && kk + 8 <= E) {
                    v = *(const u16x8*)src;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (kk + j < E) v[j] = src[j];
                }
            }
            xa[fm][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }

    // per-lane state of rows row_base + fm*16 + lg*4 + r
    float sm[2][4], ss[2][4], labv[2][4];
    int lab[2][4];
    float tv[2][4][KC];
    int ti[2][4][KC];
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row_base + fm * 16 + lg * 4 + r;
            sm[fm][r] = NEG_BIG;
            ss[fm][r] = 0.f;
            labv[fm][r] = 0.f;
            lab[fm][r] = (labels && row < M) ? (int)labels[row] : -1;
#pragma unroll
            for (int i = 0; i < KC; ++i) {
                tv[fm][r][i] = -INFINITY;
                ti[fm][r][i] = NO_COL;
            }
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
        // fold the 32x64 logits into the online state and the lists
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
                    if (z > tv[fm][r][KC - 1]) {
                        // sorted insert; slot i takes its upper neighbour
                        // where z passes that one too
                        bool g[KC];
#pragma unroll
                        for (int i = 0; i < KC; ++i) g[i] = z > tv[fm][r][i];
#pragma unroll
                        for (int i = KC - 1; i > 0; --i) {
                            tv[fm][r][i] = g[i - 1] ? tv[fm][r][i - 1]
                                         : g[i] ? z : tv[fm][r][i];
                            ti[fm][r][i] = g[i - 1] ? ti[fm][r][i - 1]
                                         : g[i] ? col : ti[fm][r][i];
                        }
                        tv[fm][r][0] = g[0] ? z : tv[fm][r][0];
                        ti[fm][r][0] = g[0] ? col : ti[fm][r][0];
                    }
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
            // k rounds of arg-max over the 16 list heads
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                if (q < k) {   // uniform
                    float bv = tv[fm][r][0];
                    int bi = ti[fm][r][0];
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) {
                        const float ov = __shfl_xor(bv, off, WAVE);
                        const int oi = __shfl_xor(bi, off, WAVE);
                        const bool take = before(ov, oi, bv, bi);
                        bv = take ? ov : bv;
                        bi = take ? oi : bi;
                    }
                    if (row < M && lc == 0) {
                        const long o = ((long)sp * M + row) * k + q;
                        cand_v[o] = bv;
                        cand_i[o] = bi;
                    }
                    // the winner pops its head (columns are distinct
                    // across lanes; unfilled slots pop one another)
                    const bool win = ti[fm][r][0] == bi;
#pragma unroll
                    for (int i = 0; i + 1 < KC; ++i) {
                        tv[fm][r][i] = win ? tv[fm][r][i + 1] : tv[fm][r][i];
                        ti[fm][r][i] = win ? ti[fm][r][i + 1] : ti[fm][r][i];
                    }
                    tv[fm][r][KC - 1] = win ? -INFINITY : tv[fm][r][KC - 1];
                    ti[fm][r][KC - 1] = win ? NO_COL : ti[fm][r][KC - 1];
                }
            }
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

// One thread per row: log-sum-exp as in lm_head_merge_kernel, then k rounds
// over the splits' sorted candidate lists, each round taking the best
// candidate that comes after the previous winner.  Splits are visited in
// index order and a later candidate must be strictly `before` the running
// best to replace it.
__global__ void __launch_bounds__(256)
lm_head_topk_merge_kernel(const float* __restrict__ part_m,
                          const float* __restrict__ part_s,
                          const float* __restrict__ cand_v,
                          const int* __restrict__ cand_i,
                          const float* __restrict__ lab_logit,
                          float* __restrict__ top_val,
                          long* __restrict__ top_idx,
                          float* __restrict__ row_lse,
                          float* __restrict__ row_nll, int M, int splits,
                          int k) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    float m = NEG_BIG;
    for (int s = 0; s < splits; ++s) m = fmaxf(m, part_m[(long)s * M + row]);
    float sum = 0.f;
    for (int s = 0; s < splits; ++s)
        sum += part_s[(long)s * M + row]
               * __expf(part_m[(long)s * M + row] - m);
    const float lse = m + __logf(sum);
    row_lse[row] = lse;
    if (row_nll) row_nll[row] = lse - lab_logit[row];

    float pv = INFINITY;   // the previous winner; everything comes after it
    int pi = -1;
    for (int q = 0; q < k; ++q) {
        float bv = -INFINITY;
        int bi = NO_COL;
        for (int s = 0; s < splits; ++s) {
            const long o = ((long)s * M + row) * k;
            for (int i = 0; i < k; ++i) {
                const float v = cand_v[o + i];
                const int c = cand_i[o + i];
                if (before(pv, pi, v, c)) {   // the split's first one left
                    if (before(v, c, bv, bi)) { bv = v; bi = c; }
                    break;
                }
            }
        }
        top_val[(long)row * k + q] = bv;
        top_idx[(long)row * k + q] = bi;
        pv = bv;
        pi = bi;
    }
}

}  // namespace

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The host's choice of `splits` for M rows: lm_head_ce's rule, about two
// blocks per CU, but no split shorter than 20 column tiles where lm_head_ce
// stops at 10: a split has to warm its lists up and merge them at the end,
// and the sweep at M = 640, k = 5 (profiles/lm_inferbench.txt) has 26 splits
// 17 - 29 % ahead of 52 at E = 16 / 64 / 256.  Exposed so that a caller can
// pin the value it would get for another M (the engine's only_masked runs
// reproduce the full run's bits that way).
int64_t lm_head_topk_splits(int64_t M, int64_t V) {
    TORCH_CHECK(M >= 1 && V >= 1 && V < (1L << 31) - HBN);
    const long ntiles = (V + HBN - 1) / HBN;
    const long rtiles = (M + HBM - 1) / HBM;
    const long cus = at::cuda::getCurrentDeviceProperties()
                         ->multiProcessorCount;
    return std::min((2 * cus + rtiles - 1) / rtiles,
                    std::max(ntiles / 20, 1L));
}

std::vector<at::Tensor> lm_head_topk(at::Tensor x, at::Tensor packed,
                                     at::Tensor bias, at::Tensor labels,
                                     at::Tensor vocab_mask, int64_t V,
                                     int64_t E, int64_t k, int64_t splits) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2
                && x.scalar_type() == at::kBFloat16,
                "lm_head_topk: contiguous bf16 (M, E) input expected");
    TORCH_CHECK(E >= 1 && E <= 256 && x.size(1) == E && V >= 1
                && V < (1L << 31) - HBN, "lm_head_topk: 1 <= E <= 256");
    TORCH_CHECK(k >= 1 && k <= MAX_K && k <= V,
                "lm_head_topk: 1 <= k <= 8 and k <= V");
    const long Ml = x.size(0);
    TORCH_CHECK(Ml >= 1 && Ml < (1L << 31) - HBM, "lm_head_topk: bad M");
    const int M = (int)Ml;
    const int Ep = round_up((int)E, HBK), Vp = round_up((int)V, HBN);
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous()
                && packed.scalar_type() == at::kBFloat16
                && packed.numel() == (long)Vp * Ep,
                "lm_head_topk: weight was not packed for this shape");
    // an empty tensor stands for "absent", as in the other ops
    const bool has_bias = bias.defined() && bias.numel() > 0;
    const bool has_mask = vocab_mask.defined() && vocab_mask.numel() > 0;
    const bool has_lab = labels.defined() && labels.numel() > 0;
    if (has_lab)
        TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                    && labels.scalar_type() == at::kLong
                    && labels.numel() == M,
                    "lm_head_topk: (M,) int64 labels expected");
    if (has_bias)
        TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat
                    && bias.is_contiguous() && bias.numel() == V);
    if (has_mask)
        TORCH_CHECK(vocab_mask.is_cuda()
                    && vocab_mask.scalar_type() == at::kFloat
                    && vocab_mask.is_contiguous() && vocab_mask.numel() == V);
    const int ntiles = Vp / HBN;
    const int rtiles = (M + HBM - 1) / HBM;
    if (splits <= 0) splits = lm_head_topk_splits(Ml, V);
    if (splits > ntiles) splits = ntiles;
    TORCH_CHECK(splits >= 1 && splits <= 65535);
    auto opts = x.options().dtype(at::kFloat);
    auto part = at::empty({2, (long)splits, Ml}, opts);
    auto cand_v = at::empty({(long)splits, Ml, (long)k}, opts);
    auto cand_i = at::empty({(long)splits, Ml, (long)k},
                            opts.dtype(at::kInt));
    auto lab_logit = at::empty({has_lab ? Ml : 0}, opts);
    auto top_val = at::empty({Ml, (long)k}, opts);
    auto top_idx = at::empty({Ml, (long)k}, opts.dtype(at::kLong));
    auto row_lse = at::empty({Ml}, opts);
    auto row_nll = at::empty({has_lab ? Ml : 0}, opts);
    float* pm = part.data_ptr<float>();
    float* ps = pm + (long)splits * Ml;
    auto stream = at::hip::getCurrentHIPStream();
    const float* bp = has_bias ? bias.data_ptr<float>() : nullptr;
    const float* mp = has_mask ? vocab_mask.data_ptr<float>() : nullptr;
    const long* lp = has_lab ? labels.data_ptr<long>() : nullptr;
    float* llp = has_lab ? lab_logit.data_ptr<float>() : nullptr;
    const dim3 grid((unsigned)rtiles, (unsigned)splits);
#define LAUNCH_TOPK(KP, KC)                                                   \
    hipLaunchKernelGGL((lm_head_topk_kernel<KP, KC>), grid, dim3(256), 0,     \
                       stream, (const u16*)x.data_ptr(),                      \
                       (const u16*)packed.data_ptr(), bp, mp, lp, pm, ps,     \
                       cand_v.data_ptr<float>(), cand_i.data_ptr<int>(), llp, \
                       M, (int)E, Ep, (int)V, ntiles, (int)k)
    // list capacities: 1 (arg-max), 3, 5 (the fill-mask default), 8
#define LAUNCH_TOPK_K(KP)                                                     \
    do {                                                                      \
        if (k <= 1) LAUNCH_TOPK(KP, 1);                                       \
        else if (k <= 3) LAUNCH_TOPK(KP, 3);                                  \
        else if (k <= 5) LAUNCH_TOPK(KP, 5);                                  \
        else LAUNCH_TOPK(KP, 8);                                              \
    } while (0)
    if (Ep <= 32) LAUNCH_TOPK_K(32);
    else if (Ep <= 64) LAUNCH_TOPK_K(64);
    else if (Ep <= 128) LAUNCH_TOPK_K(128);
    else LAUNCH_TOPK_K(256);
#undef LAUNCH_TOPK_K
#undef LAUNCH_TOPK
    hipLaunchKernelGGL(lm_head_topk_merge_kernel,
                       dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream,
                       pm, ps, cand_v.data_ptr<float>(),
                       cand_i.data_ptr<int>(), llp,
                       top_val.data_ptr<float>(), top_idx.data_ptr<long>(),
                       row_lse.data_ptr<float>(),
                       has_lab ? row_nll.data_ptr<float>() : nullptr, M,
                       (int)splits, (int)k);
    return {top_val, top_idx, row_lse, row_nll};
}
