// Vocabulary projection of the masked-LM head in one pass over the
// vocabulary, with the (M, V) logits never written to memory and never
// rounded to bf16.  One kernel, lm_head_kernel<KP, KC>, serves both entry
// points:
//   lm_head_ce    (KC == 0)  row_lse[i] = logsumexp_j(x_i . W_j + b_j) and
//                            row_nll[i] = row_lse[i] - logit[i, label_i];
//   lm_head_topk  (KC >= 1)  the same, plus the k <= KC largest logits of
//                            every row and their columns (fill-mask).
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
//     logit is exactly 0 (bias included) and still takes part in the softmax
//     and in the top-k.  Padded columns j >= V are given the logit -inf and
//     take no part: -inf never beats a list entry, so they can not be
//     returned.
//   - KC >= 1: a lane meets its columns in ascending order and keeps, per
//     row, a list of the KC best (value, column) pairs in registers, sorted by
//     value descending and, for equal values, column ascending.  A new logit
//     is tested against the list's last value only (strict >, so an equal
//     later column never displaces an earlier one); the insertion itself is a
//     branch that is rarely taken once the list has warmed up.  Unfilled
//     slots hold (-inf, INT_MAX); they sort behind every finite logit (logits
//     are assumed finite).  After the loop the 16 lanes of a row are merged by
//     k rounds of a 16-lane arg-max over the list heads ((value desc, column
//     asc) is a total order, so every lane sees the same winner); the winning
//     lane pops its head.  Lane 0 of the group writes the split's k
//     candidates.
//   - The vocabulary is cut into `splits` contiguous runs of column tiles
//     (grid.y).  Every split writes its per-row (max, sum-exp) and its k
//     candidates to a workspace and a second kernel merges the splits in
//     index order.  The label's logit is written by the one lane that owns
//     that column.  No atomics: for a given `splits` all outputs are
//     bit-reproducible.
//   - Cross-entropy is the KC == 0 instantiation, not a second kernel: the
//     two list sections sit under `if constexpr (KC > 0)`, and a device-only
//     compile shows the KC == 0 code to be the former stand-alone CE kernel's
//     instruction for instruction, with the same register counts, up to the
//     position of one kernel-argument load in the prologue
//     (profiles/NOTES.md, "One LM head kernel").  The lists' register
//     pressure does not reach the instantiation that has none.
//
// Fragment layout of mfma_f32_16x16x32_bf16: see conv_infer.hip.
#include "common.h"

#include <climits>

namespace {

typedef unsigned short u16;

constexpr int HBM = 128;   // rows per block
constexpr int HBN = 64;    // columns per tile (V padding of the packed weight)
constexpr int HBK = 32;    // MFMA K (E padding of the packed weight)
constexpr float NEG_BIG = -1e30f;
constexpr int NO_COL = INT_MAX;   // column of an unfilled list slot
constexpr int MAX_K = 8;

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

// (va, ia) comes before (vb, ib): larger value, then lower column
__device__ __forceinline__ bool before(float va, int ia, float vb, int ib) {
    return va > vb || (va == vb && ia < ib);
}

// Blocks per CU asked of the compiler.  At KP = 256 the mainloop alone takes
// 238 registers (KC = 0), so with 8 rows x KC (value, column) pairs on top
// two blocks per CU (256 registers) spill into scratch inside the vocabulary
// loop.  Measured at M = 32768, E = 256 (profiles/lm_inferbench.txt, "blocks
// per CU"): one block per CU (512 registers, no scratch) is 1.4x faster at
// KC = 5 and 2.4x at KC = 8, and 1.4x slower at KC = 1, whose spill is 28
// bytes; KP = 64 is faster with two blocks at every KC.  KC = 3 at KP = 256
// and all of KP = 128 were not measured and keep two blocks.
constexpr int min_blocks(int KP, int KC) {
    return KP == 256 && KC >= 5 ? 1 : 2;
}

// grid: (row tiles, splits).  KP: compile-time K capacity (>= Ep), it sizes
// the LDS tile and the register-resident x fragments.  KC: capacity of the
// per-lane lists (>= k); 0 is cross-entropy only, which has no lists, writes
// no candidates and requires labels.
template <int KP, int KC>
__global__ void __launch_bounds__(256, min_blocks(KP, KC))
lm_head_kernel(const u16* __restrict__ x, const u16* __restrict__ wp,
               const float* __restrict__ bias, const float* __restrict__ vmask,
               const long* __restrict__ labels, float* __restrict__ part_m,
               float* __restrict__ part_s, float* __restrict__ cand_v,
               int* __restrict__ cand_i, float* __restrict__ lab_logit, int M,
               int E, int Ep, int V, int ntiles, int k) {
    constexpr int KS = KP / HBK;          // k-steps
    constexpr int LDK = KP + 8;           // padded k-stride of the LDS tile
    constexpr int CPR = KP / 8;           // 16-byte chunks per W row
    constexpr int NLD = HBN * CPR / 256;  // chunks per thread per tile
    constexpr int KL = KC > 0 ? KC : 1;   // declared list length
    static_assert(NLD >= 1 && NLD * 256 == HBN * CPR, "loader mapping");
    static_assert(KC >= 0 && KC <= MAX_K, "list capacity");
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
    float tv[2][4][KL];
    int ti[2][4][KL];
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row_base + fm * 16 + lg * 4 + r;
            sm[fm][r] = NEG_BIG;
            ss[fm][r] = 0.f;
            labv[fm][r] = 0.f;
            if constexpr (KC > 0) {
                lab[fm][r] = (labels && row < M) ? (int)labels[row] : -1;
#pragma unroll
                for (int i = 0; i < KC; ++i) {
                    tv[fm][r][i] = -INFINITY;
                    ti[fm][r][i] = NO_COL;
                }
            } else {
                lab[fm][r] = row < M ? (int)labels[row] : -1;
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
                    if constexpr (KC > 0) {
                        if (z > tv[fm][r][KC - 1]) {
                            // sorted insert; slot i takes its upper neighbour
                            // where z passes that one too
                            bool g[KC];
#pragma unroll
                            for (int i = 0; i < KC; ++i)
                                g[i] = z > tv[fm][r][i];
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
            if constexpr (KC > 0) {
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
                            tv[fm][r][i] = win ? tv[fm][r][i + 1]
                                               : tv[fm][r][i];
                            ti[fm][r][i] = win ? ti[fm][r][i + 1]
                                               : ti[fm][r][i];
                        }
                        tv[fm][r][KC - 1] = win ? -INFINITY
                                                : tv[fm][r][KC - 1];
                        ti[fm][r][KC - 1] = win ? NO_COL : ti[fm][r][KC - 1];
                    }
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

// One thread per row: the splits' (max, sum-exp) merged in index order, then
// k rounds over the splits' sorted candidate lists, each round taking the
// best candidate that comes after the previous winner.  Splits are visited in
// index order and a later candidate must be strictly `before` the running
// best to replace it.  k == 0 (cross-entropy only) runs no round and leaves
// the candidate and top pointers alone; row_nll is null without labels.
__global__ void __launch_bounds__(256)
lm_head_merge_kernel(const float* __restrict__ part_m,
                     const float* __restrict__ part_s,
                     const float* __restrict__ cand_v,
                     const int* __restrict__ cand_i,
                     const float* __restrict__ lab_logit,
                     float* __restrict__ top_val, long* __restrict__ top_idx,
                     float* __restrict__ row_lse, float* __restrict__ row_nll,
                     int M, int splits, int k) {
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

// The host's choice of `splits` for M rows: about two blocks per CU, but no
// split shorter than `min_tiles` column tiles.  Cross-entropy stops at 10:
// below that the per-block prologue (x fragments) and the merge outweigh the
// extra parallelism (splits sweep in profiles/lm_inferbench.txt).  Top-k
// stops at 20: a split also has to warm its lists up and merge them at the
// end, and the sweep at M = 640, k = 5 has 26 splits 17 - 29 % ahead of 52 at
// E = 16 / 64 / 256.
static long default_splits(long M, long V, long min_tiles) {
    const long ntiles = (V + HBN - 1) / HBN;
    const long rtiles = (M + HBM - 1) / HBM;
    const long cus = at::cuda::getCurrentDeviceProperties()
                         ->multiProcessorCount;
    return std::min((2 * cus + rtiles - 1) / rtiles,
                    std::max(ntiles / min_tiles, 1L));
}

// Exposed so that a caller can pin the value lm_head_topk would choose for
// another M (the engine's only_masked runs reproduce the full run's bits
// that way).
int64_t lm_head_topk_splits(int64_t M, int64_t V) {
    TORCH_CHECK(M >= 1 && V >= 1 && V < (1L << 31) - HBN);
    return default_splits(M, V, 20);
}

// Both entry points: checks, workspace, the main kernel and the merge.
// k == 0 is cross-entropy only and requires labels; k >= 1 accepts none.
// Returns {top_val, top_idx, row_lse, row_nll}, the first two undefined at
// k == 0 and row_nll empty without labels.
static std::vector<at::Tensor> lm_head_run(
        const char* name, at::Tensor x, at::Tensor packed, at::Tensor bias,
        at::Tensor labels, at::Tensor vocab_mask, int64_t V, int64_t E,
        int64_t k, int64_t splits, long min_tiles) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2
                && x.scalar_type() == at::kBFloat16, name,
                ": contiguous bf16 (M, E) input expected");
    TORCH_CHECK(E >= 1 && E <= 256 && x.size(1) == E && V >= 1
                && V < (1L << 31) - HBN, name, ": 1 <= E <= 256");
    TORCH_CHECK(k >= 0 && k <= MAX_K && k <= V, name,
                ": 1 <= k <= 8 and k <= V");
    const long Ml = x.size(0);
    TORCH_CHECK(Ml >= 1 && Ml < (1L << 31) - HBM, name, ": bad M");
    const int M = (int)Ml;
    const int Ep = round_up((int)E, HBK), Vp = round_up((int)V, HBN);
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous()
                && packed.scalar_type() == at::kBFloat16
                && packed.numel() == (long)Vp * Ep, name,
                ": weight was not packed for this shape");
    // an empty tensor stands for "absent", as in the other ops
    const bool has_bias = bias.defined() && bias.numel() > 0;
    const bool has_mask = vocab_mask.defined() && vocab_mask.numel() > 0;
    const bool has_lab = k == 0 || (labels.defined() && labels.numel() > 0);
    if (has_lab)
        TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                    && labels.scalar_type() == at::kLong
                    && labels.numel() == M, name,
                    ": (M,) int64 labels expected");
    if (has_bias)
        TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat
                    && bias.is_contiguous() && bias.numel() == V);
    if (has_mask)
        TORCH_CHECK(vocab_mask.is_cuda()
                    && vocab_mask.scalar_type() == at::kFloat
                    && vocab_mask.is_contiguous() && vocab_mask.numel() == V);
    const int ntiles = Vp / HBN;
    const int rtiles = (M + HBM - 1) / HBM;
    if (splits <= 0) splits = default_splits(Ml, V, min_tiles);
    if (splits > ntiles) splits = ntiles;
    TORCH_CHECK(splits >= 1 && splits <= 65535);
    auto opts = x.options().dtype(at::kFloat);
    auto part = at::empty({2, (long)splits, Ml}, opts);
    auto lab_logit = at::empty({has_lab ? Ml : 0}, opts);
    auto row_lse = at::empty({Ml}, opts);
    auto row_nll = at::empty({has_lab ? Ml : 0}, opts);
    at::Tensor cand_v, cand_i, top_val, top_idx;
    float *cvp = nullptr, *tvp = nullptr;
    int* cip = nullptr;
    long* tip = nullptr;
    if (k > 0) {
        cand_v = at::empty({(long)splits, Ml, (long)k}, opts);
        cand_i = at::empty({(long)splits, Ml, (long)k}, opts.dtype(at::kInt));
        top_val = at::empty({Ml, (long)k}, opts);
        top_idx = at::empty({Ml, (long)k}, opts.dtype(at::kLong));
        cvp = cand_v.data_ptr<float>();
        cip = cand_i.data_ptr<int>();
        tvp = top_val.data_ptr<float>();
        tip = top_idx.data_ptr<long>();
    }
    float* pm = part.data_ptr<float>();
    float* ps = pm + (long)splits * Ml;
    auto stream = at::hip::getCurrentHIPStream();
    const float* bp = has_bias ? bias.data_ptr<float>() : nullptr;
    const float* mp = has_mask ? vocab_mask.data_ptr<float>() : nullptr;
    const long* lp = has_lab ? labels.data_ptr<long>() : nullptr;
    float* llp = has_lab ? lab_logit.data_ptr<float>() : nullptr;
    const dim3 grid((unsigned)rtiles, (unsigned)splits);
#define LAUNCH_HEAD(KP, KC)                                                   \
    hipLaunchKernelGGL((lm_head_kernel<KP, KC>), grid, dim3(256), 0, stream,  \
                       (const u16*)x.data_ptr(),                              \
                       (const u16*)packed.data_ptr(), bp, mp, lp, pm, ps,     \
                       cvp, cip, llp, M, (int)E, Ep, (int)V, ntiles, (int)k)
    // list capacities: 0 (cross-entropy), 1 (arg-max), 3, 5 (the fill-mask
    // default), 8
#define LAUNCH_HEAD_K(KP)                                                     \
    do {                                                                      \
        if (k == 0) LAUNCH_HEAD(KP, 0);                                       \
        else if (k <= 1) LAUNCH_HEAD(KP, 1);                                  \
        else if (k <= 3) LAUNCH_HEAD(KP, 3);                                  \
        else if (k <= 5) LAUNCH_HEAD(KP, 5);                                  \
        else LAUNCH_HEAD(KP, 8);                                              \
    } while (0)
    if (Ep <= 32) LAUNCH_HEAD_K(32);
    else if (Ep <= 64) LAUNCH_HEAD_K(64);
    else if (Ep <= 128) LAUNCH_HEAD_K(128);
    else LAUNCH_HEAD_K(256);
#undef LAUNCH_HEAD_K
#undef LAUNCH_HEAD
    hipLaunchKernelGGL(lm_head_merge_kernel,
                       dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream,
                       pm, ps, cvp, cip, llp, tvp, tip,
                       row_lse.data_ptr<float>(),
                       has_lab ? row_nll.data_ptr<float>() : nullptr, M,
                       (int)splits, (int)k);
    return {top_val, top_idx, row_lse, row_nll};
}

std::vector<at::Tensor> lm_head_ce(at::Tensor x, at::Tensor packed,
                                   at::Tensor bias, at::Tensor labels,
                                   at::Tensor vocab_mask, int64_t V,
                                   int64_t E, int64_t splits) {
    auto out = lm_head_run("lm_head_ce", x, packed, bias, labels, vocab_mask,
                           V, E, 0, splits, 10);
    return {out[3], out[2]};   // row_nll, row_lse
}

std::vector<at::Tensor> lm_head_topk(at::Tensor x, at::Tensor packed,
                                     at::Tensor bias, at::Tensor labels,
                                     at::Tensor vocab_mask, int64_t V,
                                     int64_t E, int64_t k, int64_t splits) {
    TORCH_CHECK(k >= 1, "lm_head_topk: 1 <= k <= 8 and k <= V");
    return lm_head_run("lm_head_topk", x, packed, bias, labels, vocab_mask, V,
                       E, k, splits, 20);
}
