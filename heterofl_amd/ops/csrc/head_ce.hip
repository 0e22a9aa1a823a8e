// Classifier tail of the batched vision step in two launches: avg-pool +
// per-client linear + masked CE (+ metrics) forward, and masked-CE backward +
// head backward.  Every value keeps the arithmetic chain it has in head.hip
// and masked_ce.hip (same operands, same order, the dot products spelled as
// the fmas those kernels compile to), so the outputs have their bits; what
// changes is who computes a value and how the bytes move:
//   - feat is read and dfeat written 16 bytes at a time where a plane is a
//     multiple of 16 bytes and the bases are aligned (element path otherwise);
//   - the client's w (J, C) is staged in LDS with coalesced loads, rows padded
//     by one float so lanes that differ in n or j hit different banks;
//   - the forward runs one 1024-lane block per client (the CE needs the
//     client's complete score rows; nothing depends on block arrival order),
//     the backward a grid over (client, 32-channel slice), each block
//     recomputing the client's N x J dscores, which are never written out.
// Envelope (head_ce_route): both LDS stages within 64 KB,
//   fwd ((N + J) * (C + 1) + N * J) * 4,  bwd (N * J + J * 32) * 4.
// Outside it, or with HETEROFL_STEP_FUSED=0, the entries run the old chain
// head_fwd -> masked_ce_fwd and masked_ce_bwd -> head_bwd.
#include "common.h"

constexpr int HCE_FWD_THREADS = 1024;
constexpr int HCE_CS = 32;            // channels per backward block
constexpr long HCE_LDS = 64 * 1024;

template <typename T, bool VEC>
__global__ void __launch_bounds__(HCE_FWD_THREADS)
head_ce_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ w,
                   const float* __restrict__ b,
                   const long* __restrict__ labels,
                   const float* __restrict__ mask, float* __restrict__ pooled,
                   float* __restrict__ scores, float* __restrict__ losses,
                   float* __restrict__ metrics, int N, int R, int C, int HW,
                   int J) {
    const int r = blockIdx.x;
    const int CP = C + 1;
    extern __shared__ float lds[];
    float* sp = lds;              // (N, CP) pooled
    float* sw = sp + N * CP;      // (J, CP) this client's weight
    float* ss = sw + J * CP;      // (N, J) scores
    const float* wr0 = w + (long)r * J * C;
    for (int e = threadIdx.x; e < J * C; e += blockDim.x) {
        const int j = e / C, c = e - j * C;
        sw[j * CP + c] = wr0[e];
    }
    const float inv_hw = 1.f / HW;
    for (int e = threadIdx.x; e < N * C; e += blockDim.x) {
        const int n = e / C, c = e - n * C;
        const T* src = feat + ((long)n * R * C + (long)r * C + c) * HW;
        float s = 0.f;
        if (VEC) {
            constexpr int V = 16 / sizeof(T);
            const uint4* src4 = (const uint4*)src;
            for (int v = 0; v < HW / V; ++v) {
                float f[V];
                unpack16<T>(src4[v], f);
#pragma unroll
                for (int k = 0; k < V; ++k) s += f[k];
            }
        } else {
            for (int i = 0; i < HW; ++i) s += ld_f32(src + i);
        }
        const float m = s * inv_hw;
        sp[n * CP + c] = m;
        pooled[((long)n * R + r) * C + c] = m;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < N * J; e += blockDim.x) {
        const int n = e / J, j = e - n * J;
        const float* wr = sw + j * CP;
        const float* pr = sp + n * CP;
        float s = b ? b[r * J + j] : 0.f;
        for (int c = 0; c < C; ++c) s = __fmaf_rn(pr[c], wr[c], s);
        ss[e] = s;
        scores[((long)n * R + r) * J + j] = s;
    }
    __syncthreads();
    // masked_ce_fwd_kernel on the LDS score rows: a lane per sample
    if (threadIdx.x >= WAVE) return;
    const int lane = threadIdx.x;
    float loss = 0.f;
    int correct = 0;
    for (int n = lane; n < N; n += WAVE) {
        const float* s = ss + n * J;
        const long y = labels[(long)n * R + r];
        float mx = -1e30f;
        int arg = 0;
        for (int c = 0; c < J; ++c) {
            float v = s[c];
            if (mask) v = mask[r * J + c] != 0.f ? v : 0.f;
            if (v > mx) { mx = v; arg = c; }
        }
        float lse = 0.f;
        for (int c = 0; c < J; ++c) {
            float v = s[c];
            if (mask) v = mask[r * J + c] != 0.f ? v : 0.f;
            lse += __expf(v - mx);
        }
        lse = mx + __logf(lse);
        float vy = s[y];
        if (mask) vy = mask[r * J + y] != 0.f ? vy : 0.f;
        loss += lse - vy;
        correct += (arg == y);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        loss += __shfl_down(loss, off, WAVE);
        correct += __shfl_down(correct, off, WAVE);
    }
    if (lane == 0) {
        losses[r] = loss / N;
        if (metrics) {
            metrics[r * 3 + 0] += loss;
            metrics[r * 3 + 1] += correct;
            metrics[r * 3 + 2] += N;
        }
    }
}

// grid (R, ceil(C / HCE_CS)); up is read through its stride
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
head_ce_bwd_kernel(const float* __restrict__ up, long up_stride,
                   const float* __restrict__ scores,
                   const long* __restrict__ labels,
                   const float* __restrict__ mask,
                   const float* __restrict__ pooled,
                   const float* __restrict__ w, float* __restrict__ dw,
                   float* __restrict__ db, T* __restrict__ dfeat, int N,
                   int R, int C, int HW, int J) {
    const int r = blockIdx.x;
    const int c0 = blockIdx.y * HCE_CS;
    const int cs = min(HCE_CS, C - c0);
    extern __shared__ float lds[];
    float* ds = lds;              // (N, J) dscores of this client
    float* sw = ds + N * J;       // (J, HCE_CS) weight slice
    for (int e = threadIdx.x; e < J * cs; e += blockDim.x) {
        const int j = e / cs, c = e - j * cs;
        sw[j * HCE_CS + c] = w[((long)r * J + j) * C + c0 + c];
    }
    // masked_ce_bwd_kernel, a lane per score row
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const long i = (long)n * R + r;
        const float* s = scores + i * J;
        float* dsr = ds + n * J;
        const long y = labels[i];
        float mx = -1e30f;
        for (int c = 0; c < J; ++c) {
            float v = s[c];
            if (mask) v = mask[r * J + c] != 0.f ? v : 0.f;
            mx = fmaxf(mx, v);
        }
        float denom = 0.f;
        for (int c = 0; c < J; ++c) {
            float v = s[c];
            if (mask) v = mask[r * J + c] != 0.f ? v : 0.f;
            denom += __expf(v - mx);
        }
        const float scale = up[r * up_stride] / N;
        for (int c = 0; c < J; ++c) {
            float v = s[c];
            bool live = true;
            if (mask) live = mask[r * J + c] != 0.f;
            v = live ? v : 0.f;
            float g = __expf(v - mx) / denom - (c == y ? 1.f : 0.f);
            dsr[c] = live ? scale * g : 0.f;
        }
    }
    __syncthreads();
    // head_bwd_kernel's three sums, n and j ascending
    for (int e = threadIdx.x; e < J * cs; e += blockDim.x) {
        const int j = e / cs, c = c0 + e - j * cs;
        float s = 0.f;
        for (int n = 0; n < N; ++n)
            s = __fmaf_rn(ds[n * J + j], pooled[((long)n * R + r) * C + c], s);
        dw[((long)r * J + j) * C + c] = s;
    }
    if (db && blockIdx.y == 0) {
        for (int j = threadIdx.x; j < J; j += blockDim.x) {
            float s = 0.f;
            for (int n = 0; n < N; ++n) s += ds[n * J + j];
            db[r * J + j] = s;
        }
    }
    const float inv_hw = 1.f / HW;
    for (int e = threadIdx.x; e < N * cs; e += blockDim.x) {
        const int n = e / cs, c = e - n * cs;
        float s = 0.f;
        for (int j = 0; j < J; ++j)
            s = __fmaf_rn(ds[n * J + j], sw[j * HCE_CS + c], s);
        const float g = s * inv_hw;
        T* dst = dfeat + ((long)n * R * C + (long)r * C + c0 + c) * HW;
        if (VEC) {
            constexpr int V = 16 / sizeof(T);
            float f[V];
#pragma unroll
            for (int k = 0; k < V; ++k) f[k] = g;
            const uint4 q = pack16<T>(f);
            uint4* dst4 = (uint4*)dst;
            for (int v = 0; v < HW / V; ++v) dst4[v] = q;
        } else {
            for (int i = 0; i < HW; ++i) st_f32(dst + i, g);
        }
    }
}

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

std::vector<at::Tensor> head_fwd(at::Tensor feat, at::Tensor w, at::Tensor b,
                                 int64_t R);
std::vector<at::Tensor> head_bwd(at::Tensor dscores, at::Tensor pooled,
                                 at::Tensor w, int64_t R, int64_t H,
                                 int64_t W, bool bf16_feat, bool want_db);
std::vector<at::Tensor> masked_ce_fwd(at::Tensor scores, at::Tensor labels,
                                      at::Tensor mask, at::Tensor metrics);
at::Tensor masked_ce_bwd(at::Tensor scores, at::Tensor labels, at::Tensor mask,
                         at::Tensor up);

// HETEROFL_STEP_FUSED=0 (read on every call): the step's fused tail, batch
// gather and BN-backward add fall back to the kernels they replace.
bool step_fused_on() {
    const char* e = std::getenv("HETEROFL_STEP_FUSED");
    return !(e && e[0] == '0');
}

enum HceRoute { HCE_VEC, HCE_ELEM, HCE_CHAIN };

// an absent optional argument arrives as an empty tensor
static bool present(const at::Tensor& t) {
    return t.defined() && t.numel() > 0;
}

static HceRoute hce_route(long N, long C, long HW, long J, int esz,
                          bool aligned) {
    if (!step_fused_on()) return HCE_CHAIN;
    if (N < 1 || C < 1 || J < 1 || HW < 1) return HCE_CHAIN;
    const long fwd = ((N + J) * (C + 1) + N * J) * 4;
    const long bwd = (N * J + J * HCE_CS) * 4;
    if (fwd > HCE_LDS || bwd > HCE_LDS) return HCE_CHAIN;
    return aligned && (HW * esz) % 16 == 0 ? HCE_VEC : HCE_ELEM;
}

// 'vec' / 'elem': the fused kernels with 16-byte or element-wise feat/dfeat
// accesses; 'chain': the old four-kernel chain.  Launches nothing; R does
// not enter the decision.
std::string head_ce_route(int64_t N, int64_t R, int64_t C, int64_t HW,
                          int64_t J, int64_t elem_size, bool aligned) {
    (void)R;
    static const char* names[] = {"vec", "elem", "chain"};
    return names[hce_route(N, C, HW, J, (int)elem_size, aligned)];
}

#define DISPATCH_HCE(t, vec, ...)                                             \
    if ((t) == at::kFloat) {                                                  \
        using scalar_t = float;                                               \
        if (vec) { constexpr bool kVec = true; __VA_ARGS__; }                 \
        else { constexpr bool kVec = false; __VA_ARGS__; }                    \
    } else if ((t) == at::kBFloat16) {                                        \
        using scalar_t = __hip_bfloat16;                                      \
        if (vec) { constexpr bool kVec = true; __VA_ARGS__; }                 \
        else { constexpr bool kVec = false; __VA_ARGS__; }                    \
    } else { TORCH_CHECK(false, "unsupported dtype"); }

// feat (N, R*C, H, W), w (R, J, C), b (R, J) or undefined, labels (N, R),
// mask (R, J) or undefined, metrics (R, 3) or undefined (accumulated into)
// -> losses (R,), pooled (N, R, C), scores (N, R, J)
std::vector<at::Tensor> head_ce_fwd(at::Tensor feat, at::Tensor w,
                                    at::Tensor b, at::Tensor labels,
                                    at::Tensor mask, at::Tensor metrics,
                                    int64_t R) {
    TORCH_CHECK(feat.is_cuda() && feat.is_contiguous() && w.is_contiguous());
    TORCH_CHECK(labels.is_contiguous() && labels.scalar_type() == at::kLong);
    TORCH_CHECK(w.scalar_type() == at::kFloat);
    const int N = feat.size(0);
    const int C = (int)(feat.size(1) / R);
    const int HW = feat.numel() / std::max<int64_t>(1, N * feat.size(1));
    const int J = w.size(1);
    const HceRoute route = hce_route(N, C, HW, J, (int)feat.element_size(),
                                     ptr_aligned(feat.data_ptr(), 16));
    if (route == HCE_CHAIN) {
        auto sp = head_fwd(feat, w, b, R);
        auto l = masked_ce_fwd(sp[0], labels, mask, metrics);
        return {l[0], sp[1], sp[0]};
    }
    // every pointer the kernel indexes: on the device, of the size it walks
    TORCH_CHECK(R >= 1 && feat.dim() == 4 && feat.size(1) == R * C,
                "head_ce_fwd: feat channels must be R * C");
    TORCH_CHECK(w.is_cuda() && w.dim() == 3 && w.size(0) == R &&
                    w.size(2) == C,
                "head_ce_fwd: w must be (R, J, C) on the device");
    TORCH_CHECK(labels.is_cuda() && labels.dim() == 2 &&
                    labels.size(0) == N && labels.size(1) == R,
                "head_ce_fwd: labels must be (N, R) on the device");
    TORCH_CHECK(!present(mask) || (mask.is_cuda() && mask.is_contiguous() &&
                                   mask.scalar_type() == at::kFloat &&
                                   mask.numel() == R * J),
                "head_ce_fwd: mask must be (R, J) fp32 on the device");
    TORCH_CHECK(!present(b) || (b.is_cuda() && b.is_contiguous() &&
                                b.scalar_type() == at::kFloat &&
                                b.numel() == R * J),
                "head_ce_fwd: b must be (R, J) fp32 on the device");
    TORCH_CHECK(!present(metrics) || (metrics.is_cuda() &&
                                      metrics.is_contiguous() &&
                                      metrics.scalar_type() == at::kFloat &&
                                      metrics.numel() == R * 3),
                "head_ce_fwd: metrics must be (R, 3) fp32 on the device");
    auto opts = feat.options().dtype(at::kFloat);
    auto pooled = at::empty({N, (long)R, C}, opts);
    auto scores = at::empty({N, (long)R, J}, opts);
    auto losses = at::empty({(long)R}, opts);
    auto stream = at::hip::getCurrentHIPStream();
    const int lds = (int)(((long)(N + J) * (C + 1) + (long)N * J) * 4);
    DISPATCH_HCE(feat.scalar_type(), route == HCE_VEC, {
        hipLaunchKernelGGL((head_ce_fwd_kernel<scalar_t, kVec>),
                           dim3((int)R), dim3(HCE_FWD_THREADS), lds, stream,
                           (const scalar_t*)feat.data_ptr(),
                           w.data_ptr<float>(),
                           present(b) ? b.data_ptr<float>() : nullptr,
                           labels.data_ptr<long>(),
                           present(mask) ? mask.data_ptr<float>() : nullptr,
                           pooled.data_ptr<float>(), scores.data_ptr<float>(),
                           losses.data_ptr<float>(),
                           present(metrics) ? metrics.data_ptr<float>()
                                             : nullptr,
                           N, (int)R, C, HW, J);
    });
    return {losses, pooled, scores};
}

// up (R,) with any stride -> dW (R, J, C), db (R, J) or undefined,
// dfeat (N, R*C, H, W)
std::vector<at::Tensor> head_ce_bwd(at::Tensor up, at::Tensor scores,
                                    at::Tensor labels, at::Tensor mask,
                                    at::Tensor pooled, at::Tensor w,
                                    int64_t R, int64_t H, int64_t W,
                                    bool bf16_feat, bool want_db) {
    const auto feat_dtype = bf16_feat ? at::kBFloat16 : at::kFloat;
    const int N = scores.size(0);
    const int J = scores.size(2);
    const int C = pooled.size(2);
    const int HW = (int)(H * W);
    const int esz = bf16_feat ? 2 : 4;
    HceRoute route = hce_route(N, C, HW, J, esz, true);
    if (route == HCE_CHAIN || up.scalar_type() != at::kFloat ||
        up.dim() != 1) {
        auto dsc = masked_ce_bwd(scores, labels, mask, up);
        return head_bwd(dsc, pooled, w, R, H, W, bf16_feat, want_db);
    }
    TORCH_CHECK(scores.is_cuda() && scores.is_contiguous() &&
                    scores.scalar_type() == at::kFloat && scores.dim() == 3 &&
                    scores.size(1) == R,
                "head_ce_bwd: scores must be (N, R, J) fp32 on the device");
    TORCH_CHECK(pooled.is_cuda() && pooled.is_contiguous() &&
                    pooled.scalar_type() == at::kFloat && pooled.dim() == 3 &&
                    pooled.size(0) == N && pooled.size(1) == R,
                "head_ce_bwd: pooled must be (N, R, C) fp32 on the device");
    TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                    w.scalar_type() == at::kFloat && w.dim() == 3 &&
                    w.size(0) == R && w.size(1) == J && w.size(2) == C,
                "head_ce_bwd: w must be (R, J, C) fp32 on the device");
    TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() &&
                    labels.scalar_type() == at::kLong &&
                    labels.numel() == (long)N * R,
                "head_ce_bwd: labels must be (N, R) int64 on the device");
    TORCH_CHECK(!present(mask) || (mask.is_cuda() && mask.is_contiguous() &&
                                   mask.scalar_type() == at::kFloat &&
                                   mask.numel() == R * J),
                "head_ce_bwd: mask must be (R, J) fp32 on the device");
    TORCH_CHECK(up.is_cuda() && up.size(0) == R,
                "head_ce_bwd: up must be (R,) on the device");
    auto opts = pooled.options();
    auto dw = at::empty({(long)R, J, C}, opts);
    auto db = want_db ? at::empty({(long)R, J}, opts) : at::Tensor();
    auto dfeat = at::empty({N, (long)R * C, H, W}, opts.dtype(feat_dtype));
    if (!ptr_aligned(dfeat.data_ptr(), 16)) route = HCE_ELEM;
    auto stream = at::hip::getCurrentHIPStream();
    const int lds = (int)(((long)N * J + (long)J * HCE_CS) * 4);
    const dim3 grid((int)R, (C + HCE_CS - 1) / HCE_CS);
    DISPATCH_HCE(feat_dtype, route == HCE_VEC, {
        hipLaunchKernelGGL((head_ce_bwd_kernel<scalar_t, kVec>), grid,
                           dim3(256), lds, stream, up.data_ptr<float>(),
                           (long)up.stride(0), scores.data_ptr<float>(),
                           labels.data_ptr<long>(),
                           present(mask) ? mask.data_ptr<float>() : nullptr,
                           pooled.data_ptr<float>(), w.data_ptr<float>(),
                           dw.data_ptr<float>(),
                           want_db ? db.data_ptr<float>() : nullptr,
                           (scalar_t*)dfeat.data_ptr(), N, (int)R, C, HW, J);
    });
    return {dw, db, dfeat};
}
