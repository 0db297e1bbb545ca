// Classifier head (ABI 9): SupervisedGraphSage's scores, CrossEntropyLoss and the gradients that follow (model.py:59-69, model.py:249)
// as one row-tiled kernel plus one fixed-order reduce; include/sage355.h states the semantics.
//
// Row kernel: one 256-thread block per range of SAGE_HEAD_RANGE_ROWS = 64 rows.  w_cls [C, dim] and the range's rows of emb are staged
// once in LDS with 16-byte loads (rows past n as zeros), so emb is read from HBM once and grad_emb written once.
//   scores    lane = row, wave w owns the classes c = w, w + 4, ...: per 16 bytes of the row one ds_read_b128 of emb and one (broadcast:
//             the class is wave-uniform) of w_cls per class, four FMAs each; one accumulator per class, d ascending
//   softmax   one thread per row over its <= 64 scores in LDS: argmax, max, exp, sum, then g overwrites the scores in place
//   grad_emb  one thread per (row, 16-byte column piece): sum over c ascending of g[r, c] * w_cls[c, :]
//   grad_w    one thread per (class, 16-byte column piece): sum over the range's rows ascending of g[r, c] * emb[r, :], STORED as the
//             range's partial tile; the range's loss terms are added in row order by one thread
// Reduce kernel: one thread per element of grad_w adds the partial tiles in range order; one thread adds the partial losses.
// LDS rows are padded to an odd number of 16-byte slots (the 16 lanes of a ds_read_b128 group read 16 different rows: odd slot
// stride = 16 different slots), the score rows to an odd number of floats.  Largest shape (C = 64, dim = 256): 147.25 KiB of the 160.
#include <atomic>

#include "sage_internal.h"

namespace {

constexpr int kRows = SAGE_HEAD_RANGE_ROWS;
static_assert(kRows == kWave, "the scores phase maps one row to each lane of a wave");
using V = sage_f32x4;

__host__ __device__ inline int head_ld(int dim) { return ((dim >> 2) | 1) * 4; }      // floats per LDS row of emb / w_cls
__host__ __device__ inline int head_sc(int c) { return c | 1; }                       // floats per LDS row of scores / g
size_t head_lds_bytes(int dim, int c) { return ((size_t)(c + kRows) * head_ld(dim) + (size_t)kRows * head_sc(c) + 4 * kRows) * sizeof(float); }

template <int CPT>      // classes per thread of the scores phase: 4 * CPT >= C
__global__ __launch_bounds__(256) void xent_head_kernel(const sage_head_t a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int dim = a.dim, C = a.num_classes, q4 = dim >> 2;
    const int LD = head_ld(dim), SC = head_sc(C);
    float* Ws = lds;                        // [C][LD]
    float* Es = Ws + C * LD;                // [kRows][LD]
    float* Ss = Es + kRows * LD;            // [kRows][SC]  scores, then g
    float* Ls = Ss + kRows * SC;            // [kRows]      loss terms
    float* Ms = Ls + kRows;                 // [kRows]      row maxima
    float* Zs = Ms + kRows;                 // [kRows]      sums of the exponentials
    int* Lb = reinterpret_cast<int*>(Zs + kRows);      // [kRows] label, -1 for none
    const int tid = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * kRows;
    const int rows = min(kRows, a.n - row0);

    for (int i = tid; i < C * q4; i += 256) {
        const int c = i / q4, q = i - c * q4;
        *reinterpret_cast<V*>(Ws + c * LD + q * 4) = *reinterpret_cast<const V*>(a.w_cls + (int64_t)c * a.ldw + q * 4);
    }
    for (int i = tid; i < kRows * q4; i += 256) {
        const int r = i / q4, q = i - r * q4;
        V v = {0.f, 0.f, 0.f, 0.f};
        if (r < rows) v = *reinterpret_cast<const V*>(a.emb + (int64_t)(row0 + r) * a.lde + q * 4);
        *reinterpret_cast<V*>(Es + r * LD + q * 4) = v;
    }
    __syncthreads();

    // ---- scores: s[r, c] = sum_d emb[r, d] * w[c, d], one FMA chain per (r, c), d ascending
    {
        const int r = tid & (kRows - 1), wv = tid >> 6;
        float acc[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
        const float* er = Es + r * LD;
        constexpr int kUnroll = CPT <= 2 ? 4 : CPT <= 4 ? 2 : 1;              // LDS reads of several steps in flight; the chains keep their order
#pragma unroll kUnroll
        for (int q = 0; q < q4; ++q) {
            const V e = *reinterpret_cast<const V*>(er + q * 4);
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int c = min(wv + 4 * i, C - 1);                         // a class past C recomputes the last one and is dropped below
                const V w = *reinterpret_cast<const V*>(Ws + c * LD + q * 4);
                acc[i] = fmaf(e[0], w[0], acc[i]);
                acc[i] = fmaf(e[1], w[1], acc[i]);
                acc[i] = fmaf(e[2], w[2], acc[i]);
                acc[i] = fmaf(e[3], w[3], acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < CPT; ++i)
            if (wv + 4 * i < C) Ss[r * SC + wv + 4 * i] = acc[i];
    }
    __syncthreads();

    if (a.scores) {
        for (int i = tid; i < rows * C; i += 256) {
            const int r = i / C, c = i - r * C;
            a.scores[(int64_t)(row0 + r) * a.lds + c] = Ss[r * SC + c];
        }
        __syncthreads();                                                      // g overwrites the scores below
    }

    // ---- softmax.  Per row (one thread each): argmax and max, then the sum of the exponentials, c ascending; per element (all threads):
    //      the exponentials and g = scale * (softmax - onehot), which overwrites the scores in place
    if (tid < kRows) {
        const float* s = Ss + tid * SC;
        float best = s[0];
        int arg = 0;
#pragma unroll 8
        for (int c = 1; c < C; ++c) {                                         // first maximum; the first NaN wins and stays (torch.argmax)
            const float v = s[c];
            if (!(best != best) && (v > best || v != v)) { best = v; arg = c; }
        }
        int lab = -1;                                                         // -1: no loss and no gradient from this row
        if (tid < rows) {
            if (a.pred) a.pred[row0 + tid] = arg;
            if (a.labels) {
                const int64_t l = a.labels[row0 + tid];
                if (l >= 0 && l < (int64_t)C) lab = (int)l;                   // a label outside [0, C) is never used as an index
            }
        }
        Ms[tid] = best;
        Lb[tid] = lab;
        Ls[tid] = lab >= 0 ? s[lab] - best : 0.f;
    }
    if (!a.labels) return;
    __syncthreads();
    for (int i = tid; i < kRows * C; i += 256) {
        const int r = i / C, c = i - r * C;
        Ss[r * SC + c] = expf(Ss[r * SC + c] - Ms[r]);                        // accurate expf; <= 1, so large logits cannot overflow
    }
    __syncthreads();
    if (tid < kRows) {
        const float* e = Ss + tid * SC;
        float sum = 0.f;
#pragma unroll 8
        for (int c = 0; c < C; ++c) sum += e[c];
        Zs[tid] = sum;
        Ls[tid] = Lb[tid] >= 0 ? logf(sum) - Ls[tid] : 0.f;                   // lse_r - s[r, label]
    }
    __syncthreads();
    for (int i = tid; i < kRows * C; i += 256) {
        const int r = i / C, c = i - r * C;
        const int lab = Lb[r];
        Ss[r * SC + c] = lab >= 0 ? a.scale * (Ss[r * SC + c] / Zs[r] - (c == lab ? 1.f : 0.f)) : 0.f;
    }
    __syncthreads();

    if (a.grad_emb) {
        for (int i = tid; i < rows * q4; i += 256) {
            const int r = i / q4, q = i - r * q4;
            const float* g = Ss + r * SC;
            V acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float gc = g[c];
                const V w = *reinterpret_cast<const V*>(Ws + c * LD + q * 4);
                acc[0] = fmaf(gc, w[0], acc[0]);
                acc[1] = fmaf(gc, w[1], acc[1]);
                acc[2] = fmaf(gc, w[2], acc[2]);
                acc[3] = fmaf(gc, w[3], acc[3]);
            }
            *reinterpret_cast<V*>(a.grad_emb + (int64_t)(row0 + r) * a.ldg + q * 4) = acc;
        }
    }
    if (a.part_w) {
        float* tile = a.part_w + (size_t)blockIdx.x * (size_t)(C * dim);
        for (int i = tid; i < C * q4; i += 256) {
            const int c = i / q4, q = i - c * q4;
            V acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int r = 0; r < rows; ++r) {
                const float gc = Ss[r * SC + c];
                const V e = *reinterpret_cast<const V*>(Es + r * LD + q * 4);
                acc[0] = fmaf(gc, e[0], acc[0]);
                acc[1] = fmaf(gc, e[1], acc[1]);
                acc[2] = fmaf(gc, e[2], acc[2]);
                acc[3] = fmaf(gc, e[3], acc[3]);
            }
            *reinterpret_cast<V*>(tile + c * dim + q * 4) = acc;
        }
    }
    if (a.part_loss && tid == 0) {
        float t = 0.f;                                                        // rows past n hold 0
#pragma unroll
        for (int r = 0; r < kRows; r += 4) {
            const V v = *reinterpret_cast<const V*>(Ls + r);
            t += v[0]; t += v[1]; t += v[2]; t += v[3];
        }
        a.part_loss[blockIdx.x] = t;
    }
}

// grad_w = the partial tiles added in range order, loss = scale * the partial losses added in range order.  One thread per element of
// grad_w: the loads of 64 ranges are issued together (the partials come from other XCDs' blocks, i.e. from beyond the L2), the adds keep
// the range order.  The LAST block owns the loss: its threads bring 256 partial losses at a time into LDS, thread 0 adds them in order.
__global__ __launch_bounds__(256) void xent_head_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_loss, int ranges,
                                                               int C, int dim, float scale, float* __restrict__ grad_w, int64_t ldgw,
                                                               float* __restrict__ loss) {
    constexpr int kBatch = 64;
    __shared__ __attribute__((aligned(16))) float terms[256];
    if (loss && blockIdx.x == gridDim.x - 1) {
        float t = 0.f;
        for (int k0 = 0; k0 < ranges; k0 += 256) {
            __syncthreads();
            terms[threadIdx.x] = k0 + (int)threadIdx.x < ranges ? part_loss[k0 + threadIdx.x] : 0.f;
            __syncthreads();
            if (threadIdx.x == 0) {
#pragma unroll 16
                for (int k = 0; k < 256; k += 4) {
                    const V v = *reinterpret_cast<const V*>(terms + k);
                    t += v[0]; t += v[1]; t += v[2]; t += v[3];
                }
            }
        }
        if (threadIdx.x == 0) *loss = scale * t;
        return;
    }
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (grad_w && i < C * dim) {
        const int c = i / dim, d = i - c * dim;
        const size_t tile = (size_t)(C * dim);
        const float* p = part_w + i;
        float acc = p[0];
        for (int k = 1; k < ranges; k += kBatch) {
            float v[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) v[j] = k + j < ranges ? p[(size_t)(k + j) * tile] : 0.f;
#pragma unroll
            for (int j = 0; j < kBatch; ++j)
                if (k + j < ranges) acc += v[j];
        }
        grad_w[(int64_t)c * ldgw + d] = acc;
    }
}

template <int CPT>
int launch_rows(const sage_head_t& h, int ranges, hipStream_t st) {
    const size_t lds = head_lds_bytes(h.dim, h.num_classes);
    static std::atomic<bool> configured{false};
    if (lds > 64 * 1024 && !configured.load(std::memory_order_acquire)) {
        const size_t most = head_lds_bytes(SAGE_HEAD_MAX_DIM, SAGE_HEAD_MAX_CLASSES);
        if (hipFuncSetAttribute((const void*)xent_head_kernel<CPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
            sage_set_error("xent_head: cannot reserve %zu bytes of LDS", most);
            return SAGE_ELAUNCH;
        }
        configured.store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(xent_head_kernel<CPT>, dim3(ranges), dim3(256), lds, st, h);
    SAGE_CHECK_LAUNCH("xent_head_kernel");
    return SAGE_OK;
}

int head_ranges(int n) { return (int)(((int64_t)n + kRows - 1) / kRows); }
size_t head_loss_offset(int ranges, int dim, int c) { return (size_t)ranges * (size_t)c * (size_t)dim * sizeof(float); }

}  // namespace

int sage_launch_xent_head(const sage_head_t& h, hipStream_t st) {
    const int ranges = head_ranges(h.n), cpt = (h.num_classes + 3) / 4;
    int rc;
    if (cpt <= 1) rc = launch_rows<1>(h, ranges, st);
    else if (cpt <= 2) rc = launch_rows<2>(h, ranges, st);
    else if (cpt <= 4) rc = launch_rows<4>(h, ranges, st);
    else if (cpt <= 8) rc = launch_rows<8>(h, ranges, st);
    else rc = launch_rows<16>(h, ranges, st);
    if (rc != SAGE_OK) return rc;
    if (h.grad_w || h.loss) {
        const int blocks = (h.grad_w ? sage_cdiv(h.num_classes * h.dim, 256) : 0) + (h.loss ? 1 : 0);      // the loss has the last block
        hipLaunchKernelGGL(xent_head_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const float*)h.part_w, (const float*)h.part_loss,
                           ranges, (int)h.num_classes, (int)h.dim, h.scale, h.grad_w, h.ldgw, h.loss);
        SAGE_CHECK_LAUNCH("xent_head_reduce_kernel");
    }
    return SAGE_OK;
}

extern "C" int sage_xent_head_supported(int32_t dim, int32_t num_classes) {
    return dim >= 4 && dim <= SAGE_HEAD_MAX_DIM && dim % 4 == 0 && num_classes >= 1 && num_classes <= SAGE_HEAD_MAX_CLASSES;
}

// [ranges][C * dim] partial tiles, then [ranges] partial losses, rounded up to 256 bytes
extern "C" size_t sage_xent_head_workspace_bytes(int32_t n, int32_t dim, int32_t num_classes) {
    if (n < 1 || !sage_xent_head_supported(dim, num_classes)) return 0;
    const int ranges = head_ranges(n);
    return (head_loss_offset(ranges, dim, num_classes) + (size_t)ranges * sizeof(float) + 255) / 256 * 256;
}

extern "C" int sage_xent_head(const float* emb, int64_t lde, int32_t dim, const float* w_cls, int64_t ldw, int32_t num_classes,
                              const int64_t* labels, int32_t n, float scale, float* scores, int64_t lds, int32_t* pred, float* loss,
                              float* grad_emb, int64_t ldg, float* grad_w, int64_t ldgw, void* workspace, size_t workspace_bytes,
                              sage_stream_t stream) {
    SAGE_REQUIRE(emb && w_cls && workspace, "xent_head: NULL array (emb, w_cls and workspace are required)");
    SAGE_REQUIRE(n >= 1, "xent_head: n = %d", n);
    SAGE_REQUIRE(lde >= dim && ldw >= dim && (!scores || lds >= num_classes) && (!grad_emb || ldg >= dim) && (!grad_w || ldgw >= dim),
                 "xent_head: a leading dimension is shorter than its width (dim = %d, num_classes = %d)", dim, num_classes);
    SAGE_REQUIRE(labels || !(loss || grad_emb || grad_w), "xent_head: loss / gradients requested without labels");
    const bool lds_ok = lde % 4 == 0 && ldw % 4 == 0 && (!grad_emb || ldg % 4 == 0) && (!grad_w || ldgw % 4 == 0);
    const bool aligned = sage_aligned(emb, 16) && sage_aligned(w_cls, 16) && sage_aligned(grad_emb, 16) && sage_aligned(grad_w, 16) &&
                         sage_aligned(workspace, 16);
    if (!sage_xent_head_supported(dim, num_classes) || !lds_ok || !aligned) {
        sage_set_error("xent_head: no kernel for dim = %d (4..%d, multiple of 4), num_classes = %d (1..%d), leading dimensions that are not "
                       "multiples of 4 or arrays that are not 16-byte aligned", dim, SAGE_HEAD_MAX_DIM, num_classes, SAGE_HEAD_MAX_CLASSES);
        return SAGE_EUNSUPPORTED;
    }
    const size_t need = sage_xent_head_workspace_bytes(n, dim, num_classes);
    if (need > workspace_bytes) {
        sage_set_error("xent_head: workspace %zu bytes < %zu needed", workspace_bytes, need);
        return SAGE_ENOSPACE;
    }
    sage_head_t h;
    h.emb = emb; h.lde = lde; h.dim = dim;
    h.w_cls = w_cls; h.ldw = ldw; h.num_classes = num_classes;
    h.labels = labels; h.n = n; h.scale = scale;
    h.scores = scores; h.lds = lds; h.pred = pred;
    h.grad_emb = grad_emb; h.ldg = ldg;
    h.part_w = grad_w ? (float*)workspace : nullptr;
    h.part_loss = loss ? (float*)((char*)workspace + head_loss_offset(head_ranges(n), dim, num_classes)) : nullptr;
    h.grad_w = grad_w; h.ldgw = ldgw; h.loss = loss;
    return sage_launch_xent_head(h, (hipStream_t)stream);
}
