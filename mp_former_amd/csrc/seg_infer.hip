// Inference post-processing of the mask predictions for MI355X: semantic, instance and panoptic results straight from the
// low-resolution mask logits.
//
// Reference (mask2former/maskformer_model.py:236-279 and the three *_inference functions, :301-401): the eval branch
//     masks = F.interpolate(pred_masks, (Hp, Wp), bilinear)                    fp32 [Q, Hp, Wp]   (~390 MB per COCO image)
//     masks = sem_seg_postprocess(masks, (hi, wi), H, W)   = crop + bilinear   fp32 [Q, H, W]
//     then sigmoid / "> 0" / products over whole [Q, H, W] tensors, and four .item() syncs per kept query (panoptic).
// Here every output pixel is computed from the 4 x 4 low-resolution neighbourhood behind its 2 x 2 intermediate pixels
// (both resamples composed, torch's upsample_bilinear2d index rule and weight order at each stage), so each kernel reads
// the [Q, h, w] logits once and writes only its final result.  The [Q, Hp, Wp] and [Q, H, W] intermediates never exist.
//
//   seg_softmax_kernel      softmax of the [Q, K+1] class logits -> probs [Q, K] (no-object column dropped) and the
//                           panoptic keep list (label != K and score > threshold), compacted in query order.
//   seg_product             sem_seg[c, p] = sum_q probs[q, c] * sigmoid(m_q(p)), fp32: a tile of 128 pixels x <= 192
//                           classes per workgroup, the sigmoids of 32 queries at a time staged in LDS.  ONE body with two
//                           epilogues: "put" (seg_semantic_kernel: the scores stored) and "argmax" (seg_labels_kernel, below).
//   seg_instance_kernel     per (selected entry, 1024-pixel tile): either the partial sums of sigmoid(m) * [m > 0] and
//                           [m > 0] (workspace, no atomics) or the 0/1 mask of the entry.
//   seg_instance_reduce     the partials of one entry summed in a fixed order: bitwise deterministic scores.
//   seg_panoptic_kernel     per pixel: the winning kept query (first index on ties), its sigmoid >= 0.5 bit, and the three
//                           integer areas per kept query (LDS histogram, then integer global atomics: order-independent).
//   seg_paint_kernel        int32 id map from the winner code and the host's segment lookup table.
// The results an evaluation loop consumes, without the [K, H, W] scores or the [T, H, W] masks:
//   seg_labels_kernel       int32 label map = argmax of seg_semantic_kernel's scores, bit for bit, in one launch: all classes of
//                           a pixel tile in one workgroup, running (best, index) in registers, one LDS reduction at the end.
//   seg_labels_resize       "after" mode: the [K, hi, wi] scores resized plane by plane with a running argmax per output pixel.
//   seg_confusion_kernel    (K+1)^2 int64 confusion counts of prediction x ground truth: LDS histogram per workgroup where it
//                           fits, integer global atomics otherwise.
//   seg_rle_*               instance masks as uncompressed COCO run lengths: packed bits, boundaries per tile, a fixed-order
//                           scan, scatter of the boundary positions, their differences.
// Semantic test-time augmentation (mask2former/test_time_augmentation.py): the mean over the views of an image, on the device:
//   seg_tta_accumulate_kernel   the scores of one view from its logits on the fp32 MFMA, stored / added into acc [K, H, W], plain
//                               or mirrored along W
//   seg_tta_resize_add_kernel   "after" mode: [K, hi, wi] scores resized and stored / added, plain or mirrored
//   seg_tta_finish_kernel       the division by the view count in place, or the label map of the divided sums
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <type_traits>

#include "mpf_common.h"
#include "seg_shared.h"     // the composed resampling (SegGeom, pix_geom, resample) and the run-length passes, shared with seg_video.hip

namespace {

constexpr int kSemPix = 128;       // semantic: output pixels per workgroup
constexpr int kSemQ = 32;          // semantic: queries staged per LDS round
constexpr int kMaxQ = 1024;        // panoptic LDS histogram bound

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ----------------------------------------------------------------------------------------------------------------
// class softmax + panoptic keep list; one workgroup, one wave per query row
// kept: [0] count, [1 .. Q] query of kept entry n, [1+Q .. 2Q] its label; kept_score [Q]
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void seg_softmax_kernel(const float* __restrict__ cls, int Q, int K1, float thr,
                                                         float* __restrict__ probs, float* __restrict__ max_score,
                                                         int* __restrict__ max_label, int* __restrict__ kept,
                                                         float* __restrict__ kept_score)
{
    __shared__ float s_score[kMaxQ];
    __shared__ int s_label[kMaxQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = K1 - 1;
    for (int q = wave; q < Q; q += kT / 64) {
        const float* row = cls + (int64_t)q * K1;
        float mx = -INFINITY;
        for (int c = lane; c < K1; c += 64) mx = fmaxf(mx, row[c]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float s = 0.f;
        for (int c = lane; c < K1; c += 64) s += expf(row[c] - mx);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        // max over the K+1 probabilities, first index on ties (torch max(-1))
        float best = -1.f;
        int bi = 0;
        for (int c = lane; c < K1; c += 64) {
            const float p = expf(row[c] - mx) / s;
            if (c < K) probs[(int64_t)q * K + c] = p;
            if (p > best) { best = p; bi = c; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            max_score[q] = s_score[q] = best;
            max_label[q] = s_label[q] = bi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {           // Q <= 1024: a serial compaction in query order, from LDS
        int n = 0;
        for (int q = 0; q < Q; ++q) {
            const int lab = s_label[q];
            const float sc = s_score[q];
            if (lab != K && sc > thr) {
                kept[1 + n] = q;
                kept[1 + Q + n] = lab;
                kept_score[n] = sc;
                ++n;
            }
        }
        kept[0] = n;
    }
}

// ---- the staging of the semantic product, shared by seg_product and seg_tta_accumulate_kernel: per round of kSemQ queries the
// sigmoids of the workgroup's kSemPix pixels and the probabilities of its class chunk go to LDS (ROW: the caller's row stride) ----
// geometry of the staging pixel of this thread (pixel tid & 127 of the tile at p0) -> whether the pixel lies in the plane
__device__ __forceinline__ bool stage_pixel(PixGeom& g, int64_t p0, const SegGeom& s)
{
    const int64_t pix = p0 + (threadIdx.x & (kSemPix - 1));
    const bool live = pix < (int64_t)s.H * s.W;
    pix_geom(g, live ? (int)(pix / s.W) : 0, live ? (int)(pix % s.W) : 0, s);
    return live;
}

// sig[i * ROW + pixel] = sigmoid(m_{q0 + i}(pixel)), thread = (pixel tid & 127, queries tid >> 7 + 2 i); padding queries (i >= nq)
// and pixels past the plane contribute 0 (their probabilities are 0 too)
template <int ROW, typename T>
__device__ __forceinline__ void stage_sigmoids(float* sig, const T* __restrict__ masks, int64_t stride_q, const PixGeom& g, bool live, int q0,
                                               int nq)
{
    const int sp = threadIdx.x & (kSemPix - 1);
    for (int i = threadIdx.x >> 7; i < kSemQ; i += kT / kSemPix) {
        float v = 0.f;
        if (i < nq && live) v = sigm(resample(masks + (int64_t)(q0 + i) * stride_q, g));
        sig[i * ROW + sp] = v;
    }
}

// pr[i * ROW + c] = probs[q0 + i][cbase + c] for the KC classes of the chunk, 0 past nq and past K (dense rows: the flat index,
// which the compiler does not recover from i and c)
template <int KC, int ROW>
__device__ __forceinline__ void stage_probs(float* pr, const float* __restrict__ probs, int K, int cbase, int q0, int nq)
{
    for (int e = threadIdx.x; e < kSemQ * KC; e += kT) {
        const int i = e / KC, c = e % KC;
        pr[ROW == KC ? e : i * ROW + c] = (i < nq && cbase + c < K) ? probs[(int64_t)(q0 + i) * K + cbase + c] : 0.f;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// the semantic product: score[c, p] = sum_q probs[q, c] * sigmoid(m_q(p)) for a tile of kSemPix pixels and chunks of 8 * CPT classes
// thread (pg = tid & 31, cg = tid >> 5): pixels pg*4 .. +3, classes cbase + cg*CPT .. +CPT-1.  Per chunk the sigmoids of kSemQ
// queries at a time and their probabilities are staged in LDS, and every (class, pixel) is one fmaf chain in query order: the
// scores have the same bits whatever becomes of them.  The whole body is one inlined function (a helper that took the accumulators
// by reference cost registers and scratch); the two kernels below are its instantiations.
//   put (Argmax false):  the chunk blockIdx.y is stored to out [K, H, W], four pixels of a class per thread
//   argmax (Argmax true): one workgroup owns ALL classes of its pixels and walks the chunks in a loop (the sigmoids are recomputed
//                        per chunk: K <= 192, every shipped config, is one chunk).  Each thread keeps a running (best, index) per
//                        pixel over its own classes (ascending, strict ">": the lowest index wins a tie); the 8 class groups of a
//                        pixel meet once at the end through LDS: labels[p] = argmax_c of the scores "put" would write
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int CPT, bool Argmax>
__device__ __forceinline__ void seg_product(const T* __restrict__ masks, const SegGeom s, const float* __restrict__ probs, int K,
                                            float* __restrict__ out, int* __restrict__ labels)
{
    constexpr int KC = 8 * CPT;
    __shared__ float4 sig4[kSemQ][kSemPix / 4];
    __shared__ float4 pr4[kSemQ][KC / 4];
    static_assert(2 * (kT / 32) <= kSemQ, "the final reduction of the argmax reuses the sigmoid staging");
    const int tid = threadIdx.x;
    const int Q = s.Q;
    const int64_t HW = (int64_t)s.H * s.W;
    const int64_t p0 = (int64_t)blockIdx.x * kSemPix;
    PixGeom g;
    const bool live = stage_pixel(g, p0, s);
    float* sig = (float*)sig4;
    float* pr = (float*)pr4;
    const int pg = tid & 31, cg = tid >> 5;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bidx[4] = {K, K, K, K};
    for (int cbase = Argmax ? 0 : blockIdx.y * KC; cbase < K; cbase += KC) {
        float acc[CPT][4];
#pragma unroll
        for (int j = 0; j < CPT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
        for (int q0 = 0; q0 < Q; q0 += kSemQ) {
            const int nq = min(kSemQ, Q - q0);
            __syncthreads();
            stage_sigmoids<kSemPix>(sig, masks, s.stride_q, g, live, q0, nq);
            stage_probs<KC, KC>(pr, probs, K, cbase, q0, nq);
            __syncthreads();
            for (int i = 0; i < nq; ++i) {
                const float4 sv = sig4[i][pg];
#pragma unroll
                for (int j4 = 0; j4 < CPT / 4; ++j4) {
                    const float4 pv = pr4[i][cg * (CPT / 4) + j4];
                    const float pj[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float* a = acc[j4 * 4 + u];
                        a[0] = fmaf(pj[u], sv.x, a[0]);
                        a[1] = fmaf(pj[u], sv.y, a[1]);
                        a[2] = fmaf(pj[u], sv.z, a[2]);
                        a[3] = fmaf(pj[u], sv.w, a[3]);
                    }
                }
            }
        }
        if constexpr (Argmax) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int c = cbase + cg * CPT + j;
                if (c < K) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (acc[j][i] > best[i]) { best[i] = acc[j][i]; bidx[i] = c; }
                }
            }
        } else {
            const int64_t px = p0 + pg * 4;
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int c = cbase + cg * CPT + j;
                if (c >= K) break;
                float* o = out + (int64_t)c * HW + px;
                if (px + 3 < HW && ((HW & 3) == 0)) {
                    *(float4*)o = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (px + i < HW) o[i] = acc[j][i];
                }
            }
            return;                                             // one chunk per workgroup
        }
    }
    if constexpr (Argmax) {
        // the 8 class groups of a pixel meet in the staging buffer (no LDS beyond the put form's: same occupancy)
        float (*red_v)[kSemPix] = (float (*)[kSemPix])sig;
        int (*red_i)[kSemPix] = (int (*)[kSemPix])(sig + (kT / 32) * kSemPix);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            red_v[cg][pg * 4 + i] = best[i];
            red_i[cg][pg * 4 + i] = bidx[i];
        }
        __syncthreads();
        if (tid < kSemPix && p0 + tid < HW) {
            float b = red_v[0][tid];
            int bi = red_i[0][tid];
#pragma unroll
            for (int c = 1; c < kT / 32; ++c) {
                const float v = red_v[c][tid];
                const int vi = red_i[c][tid];
                if (v > b || (v == b && vi < bi)) { b = v; bi = vi; }
            }
            labels[p0 + tid] = bi;
        }
    }
}

template <typename T, int CPT>
__global__ __launch_bounds__(kT) void seg_semantic_kernel(const T* __restrict__ masks, const SegGeom s, const float* __restrict__ probs,
                                                          int K, float* __restrict__ out)
{
    seg_product<T, CPT, false>(masks, s, probs, K, out, nullptr);
}

// (waves per SIMD: the running (best, index) pairs must not cost the small tiles the occupancy seg_semantic_kernel has there)
template <typename T, int CPT>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(CPT <= 4 ? 4 : CPT <= 12 ? 3 : 2))) void seg_labels_kernel(
    const T* __restrict__ masks, const SegGeom s, const float* __restrict__ probs, int K, int* __restrict__ labels)
{
    seg_product<T, CPT, true>(masks, s, probs, K, nullptr, labels);
}

// ----------------------------------------------------------------------------------------------------------------
// instance: entry t = blockIdx.y (query sel_q[t]), pixels blockIdx.x * kInstPix + tid + kT * i
//   masks_out == NULL: partial[t][tile] = {sum sigmoid(m) * [m > 0], count [m > 0]}
//   else:              masks_out[t][p] = m > 0 ? 1 : 0
// ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void seg_instance_kernel(const T* __restrict__ masks, const SegGeom sg, const int64_t* __restrict__ sel_q,
                                                          float* __restrict__ masks_out, float2* __restrict__ partial)
{
    const int t = blockIdx.y;
    const int W = sg.W;
    const int64_t HW = (int64_t)sg.H * W;
    const T* m = masks + sel_q[t] * sg.stride_q;
    float s = 0.f, n = 0.f;
#pragma unroll
    for (int i = 0; i < kInstPix / kT; ++i) {
        const int64_t p = (int64_t)blockIdx.x * kInstPix + threadIdx.x + kT * i;
        if (p >= HW) break;
        PixGeom g;
        pix_geom(g, (int)(p / W), (int)(p % W), sg);
        const float v = resample(m, g);
        const bool on = v > 0.f;
        if (masks_out) {
            masks_out[t * HW + p] = on ? 1.f : 0.f;
        } else if (on) {
            s += sigm(v);
            n += 1.f;
        }
    }
    if (masks_out) return;
    // fixed-order workgroup reduction: wave shuffles, then wave 0 over the 4 wave sums
    __shared__ float ws[2][kT / 64];
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        n += __shfl_xor(n, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { ws[0][wave] = s; ws[1][wave] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < kT / 64; ++i) { a += ws[0][i]; b += ws[1][i]; }
        partial[(int64_t)t * gridDim.x + blockIdx.x] = make_float2(a, b);
    }
}

// one wave per entry: lane l sums tiles l, l + 64, ... in order, then a fixed shuffle tree (no atomics: bitwise deterministic);
// scores[t] = cls_score[t] * sum / (count + 1e-6)
__global__ __launch_bounds__(kT) void seg_instance_reduce_kernel(const float2* __restrict__ partial, int tiles, int T,
                                                                 const float* __restrict__ cls_score, float* __restrict__ scores)
{
    const int t = blockIdx.x * (kT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;                                    // whole waves leave together
    float a = 0.f, b = 0.f;
    for (int i = lane; i < tiles; i += 64) {
        const float2 v = partial[(int64_t)t * tiles + i];
        a += v.x;
        b += v.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if (lane == 0) scores[t] = cls_score[t] * (a / (b + 1e-6f));
}

// ----------------------------------------------------------------------------------------------------------------
// panoptic kernel 1: one thread per pixel over the kept list (count read from the device)
//   code[p] = 2 * winner + (sigmoid(m_winner) >= 0.5);  areas [3][Q]: mask_area, original_area, intersection
// ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void seg_panoptic_kernel(const T* __restrict__ masks, const SegGeom s, const int* __restrict__ kept,
                                                          const float* __restrict__ kept_score, int* __restrict__ code,
                                                          int* __restrict__ areas)
{
    __shared__ int hist[3][kMaxQ];
    __shared__ int kq[kMaxQ];
    __shared__ float ks[kMaxQ];
    const int count = kept[0];
    for (int i = threadIdx.x; i < count; i += kT) {
        hist[0][i] = hist[1][i] = hist[2][i] = 0;
        kq[i] = kept[1 + i];
        ks[i] = kept_score[i];
    }
    __syncthreads();
    const int W = s.W;
    const int64_t HW = (int64_t)s.H * W;
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p < HW) {
        PixGeom g;
        pix_geom(g, (int)(p / W), (int)(p % W), s);
        float best = -1.f;
        int win = 0, bit = 0;
        for (int n = 0; n < count; ++n) {
            const float sg = sigm(resample(masks + (int64_t)kq[n] * s.stride_q, g));
            const float pr = ks[n] * sg;
            const int on = sg >= 0.5f;
            const unsigned long long b = __ballot(on);         // n is wave-uniform: one LDS atomic per wave, not per lane
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&hist[1][n], __popcll(b));
            if (pr > best) { best = pr; win = n; bit = on; }
        }
        if (count > 0) {
            atomicAdd(&hist[0][win], 1);
            if (bit) atomicAdd(&hist[2][win], 1);
        }
        code[p] = 2 * win + bit;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < count; i += kT)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (hist[a][i]) atomicAdd(&areas[a * s.Q + i], hist[a][i]);
}

// kernel 2: id map; lut[n] = segment id of kept entry n (0 = dropped)
__global__ __launch_bounds__(kT) void seg_paint_kernel(const int* __restrict__ code, int64_t HW, const int* __restrict__ lut,
                                                       int* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= HW) return;
    const int c = code[p];
    out[p] = (c & 1) ? lut[c >> 1] : 0;
}

// labels of the "after" mode: scores fp32 [K, hi, wi] (mpf_seg_semantic on the cropped grid) resized to [H, W] plane by plane with
// the tap() / lerp2 rule, running argmax per output pixel (first index on ties); the [K, H, W] map is never written
__global__ __launch_bounds__(kT) void seg_labels_resize_kernel(const float* __restrict__ scores, int K, int hi, int wi, int H, int W,
                                                               int* __restrict__ labels)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= HW) return;
    const Tap ty = tap((int)(p / W), hi, H), tx = tap((int)(p % W), wi, W);
    const int64_t plane = (int64_t)hi * wi;
    const int64_t o00 = (int64_t)ty.i0 * wi + tx.i0, o01 = (int64_t)ty.i0 * wi + tx.i1, o10 = (int64_t)ty.i1 * wi + tx.i0,
                  o11 = (int64_t)ty.i1 * wi + tx.i1;
    float best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < K; ++c) {
        const float* s = scores + c * plane;
        const float v = lerp2(ty.l0, ty.l1, tx.l0, tx.l1, s[o00], s[o01], s[o10], s[o11]);
        if (v > best) { best = v; bi = c; }
    }
    labels[p] = bi;
}

// ----------------------------------------------------------------------------------------------------------------
// confusion matrix: conf[(K+1) * pred + gt] += 1 over n pixels, integers only.  Each thread walks kConfRun consecutive pixels and
// merges equal neighbours (label maps are piecewise constant) before it adds.  LDS form: a per-workgroup histogram of (K+1)^2
// int32 counters in dynamic LDS, flushed with one 64-bit integer atomic per non-zero counter; global form: the merged runs go to
// conf directly.
// ----------------------------------------------------------------------------------------------------------------
constexpr int kConfT = 1024;       // threads per workgroup: 16 waves, the histogram is the only LDS user of its CU
constexpr int kConfRun = 8;        // consecutive pixels per thread
// LDS of a CU is 160 KiB (MI355X_MICROARCH.md, chip table).  One workgroup may take up to 128 KiB of it: 32 KiB stay free for a
// workgroup of another kernel on the same CU (the semantic kernels of the next image hold 24-48 KiB).  (K+1)^2 * 4 B <= 128 KiB
// is K <= 180: Cityscapes 19, COCO 133 and ADE20K 150 take the LDS form, larger class sets the global one.
constexpr size_t kConfLdsMax = 128 * 1024;

__device__ __forceinline__ int conf_cell(int pr, int g, int K, int ignore_label)
{
    const int r = (pr < 0 || pr >= K) ? K : pr;
    const int c = (g == ignore_label || g < 0 || g >= K) ? K : g;
    return r * (K + 1) + c;
}

template <bool LDS>
__global__ __launch_bounds__(kConfT) void seg_confusion_kernel(const int* __restrict__ pred, const int* __restrict__ gt, int64_t n, int K,
                                                               int ignore_label, unsigned long long* __restrict__ conf)
{
    extern __shared__ int conf_hist[];
    const int cells = (K + 1) * (K + 1);
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += kConfT) conf_hist[i] = 0;
        __syncthreads();
    }
    const int64_t nruns = (n + kConfRun - 1) / kConfRun;
    for (int64_t r = (int64_t)blockIdx.x * kConfT + threadIdx.x; r < nruns; r += (int64_t)gridDim.x * kConfT) {
        const int64_t p0 = r * kConfRun;
        const int m = (int)min((int64_t)kConfRun, n - p0);
        int cur = conf_cell(pred[p0], gt[p0], K, ignore_label), cnt = 1;
        for (int i = 1; i < m; ++i) {
            const int c = conf_cell(pred[p0 + i], gt[p0 + i], K, ignore_label);
            if (c == cur) { ++cnt; continue; }
            if (LDS) atomicAdd(&conf_hist[cur], cnt);
            else atomicAdd(&conf[cur], (unsigned long long)cnt);
            cur = c;
            cnt = 1;
        }
        if (LDS) atomicAdd(&conf_hist[cur], cnt);
        else atomicAdd(&conf[cur], (unsigned long long)cnt);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kConfT) {
            const int v = conf_hist[i];
            if (v) atomicAdd(&conf[i], (unsigned long long)v);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// instance masks as uncompressed COCO run lengths.  Position p = x * H + y (the mask flattened column-major); bit[p] = resample(m) > 0
// exactly as seg_instance_kernel decides it.  A boundary is a position whose bit differs from its predecessor's, with bit[-1] = 0:
// the counts of an instance are the differences of {0, boundaries ..., H * W}, so they start with a (possibly empty) run of zeros.
//   seg_rle_bits_kernel     64 positions per wave ballot -> one packed word; entry t = blockIdx.y
//   seg_rle_count / _scan / _scatter / _diff_kernel   the passes from the packed bits to the counts: seg_shared.h
// ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void seg_rle_bits_kernel(const T* __restrict__ masks, const SegGeom s, const int64_t* __restrict__ sel_q,
                                                          int64_t nwords, unsigned long long* __restrict__ bits)
{
    const int t = blockIdx.y;
    const int H = s.H;
    const int64_t HW = (int64_t)H * s.W;
    const T* m = masks + sel_q[t] * s.stride_q;
#pragma unroll
    for (int i = 0; i < kInstPix / kT; ++i) {
        const int64_t p = (int64_t)blockIdx.x * kInstPix + threadIdx.x + kT * i;    // wave-aligned: a wave covers one word
        bool on = false;
        if (p < HW) {
            PixGeom g;
            pix_geom(g, (int)(p % H), (int)(p / H), s);
            on = resample(m, g) > 0.f;
        }
        const unsigned long long b = __ballot(on);
        if ((threadIdx.x & 63) == 0 && (p >> 6) < nwords) bits[t * nwords + (p >> 6)] = b;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// semantic test-time augmentation (mask2former/test_time_augmentation.py:71-98): acc[K, H, W] = sum over the views of the view's
// "sem_seg", flipped back along W where the view was flipped, then one division by the number of views.
//   seg_tta_accumulate_kernel   one view straight from its logits: the product of seg_product on the fp32 matrix cores,
//                               stored or added into acc, plain or mirrored
//   seg_tta_resize_add_kernel   "after" mode: the view's [K, hi, wi] scores resized plane by plane, stored or added into acc
//   seg_tta_finish_kernel       acc /= V in place, or labels = argmax_c(acc[c] / V) with acc left alone
// mode: bit 0 = add (else store), bit 1 = hflip: output pixel (y, x) of the view lands on (y, W - 1 - x).  Every destination has
// exactly one writer (the mirror is a bijection), so "add" is a plain read-add-write.
// ----------------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTtaSigRow = kSemPix + 16;   // LDS row strides = an odd multiple of 16 floats (16 or 48 mod 64): the four k-rows of an MFMA
constexpr int kTtaPad = 16;                // fragment (lanes 0-15, 16-31, ...) fall on four different groups of 16 banks (a stride of 128: on one)
constexpr int kTtaOutRow = 36;             // epilogue staging row: 32 pixels + 4 (16-byte aligned rows, 4 row groups on 4 bank groups)

// LDS written by one wave and read back by the same wave only: program order for the compiler, no workgroup barrier (the LDS
// serves the requests of a wave in order)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// four consecutive pixels px .. px + 3 of one class plane.  vec: H * W (mirrored: W) is a multiple of 4 and the plane is 16-byte
// aligned, so the four lie in one row and, mirrored, on one aligned float4 in reverse order; otherwise pixel by pixel (a run may
// cross a row end, and the tail of the plane)
__device__ __forceinline__ void tta_put4(float* __restrict__ plane, int64_t px, int64_t HW, int W, int mode, bool vec, float4 v)
{
    const bool add = mode & 1, flip = mode & 2;
    if (vec) {
        int64_t d = px;
        if (flip) {
            const int64_t y = px / W;
            d = y * W + (W - 4 - (px - y * W));
            v = make_float4(v.w, v.z, v.y, v.x);
        }
        float4* o = (float4*)(plane + d);
        if (add) {
            const float4 a = *o;
            v = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w);
        }
        *o = v;
        return;
    }
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = px + i;
        if (p >= HW) break;
        int64_t d = p;
        if (flip) {
            const int64_t y = p / W;
            d = y * W + (W - 1 - (p - y * W));
        }
        plane[d] = add ? plane[d] + e[i] : e[i];
    }
}

// A workgroup owns kSemPix pixels x 16 * MT classes (blockIdx.y: the class chunk).  The sigmoids of kSemQ queries are staged by
// the helpers of seg_product; the product probs^T [classes x Q] * sig [Q x pixels] runs on v_mfma_f32_16x16x4_f32 with the classes on
// the A rows and the pixels on the B columns (lane l: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; C/D col = l & 15,
// row = 4 * (l >> 4) + reg).  Wave wv owns pixels 32 wv .. + 31 (two column tiles) and every class tile: 2 * MT independent
// accumulators, k ascending in query order, so each score is the fmaf chain of seg_semantic_kernel (queries past Q and classes
// past K enter as zeros).  Epilogue: one class tile at a time through LDS, so that a lane leaves with four consecutive pixels of a
// class and eight lanes cover the 128 bytes of the wave's pixels.
template <typename T, int MT>
__global__ __launch_bounds__(kT) void seg_tta_accumulate_kernel(const T* __restrict__ masks, const SegGeom s, const float* __restrict__ probs,
                                                                int K, int mode, int vec, float* __restrict__ acc)
{
    const int Q = s.Q, W = s.W;
    constexpr int KC = 16 * MT;
    constexpr int PR = KC + kTtaPad;
    __shared__ float4 sig4[kSemQ * kTtaSigRow / 4];
    __shared__ float pr[kSemQ * PR];
    static_assert((kT / 64) * 16 * kTtaOutRow <= kSemQ * kTtaSigRow, "the epilogue staging reuses the sigmoid staging");
    float* sig = (float*)sig4;
    const int tid = threadIdx.x;
    const int64_t HW = (int64_t)s.H * W;
    const int64_t p0 = (int64_t)blockIdx.x * kSemPix;
    const int cbase = blockIdx.y * KC;
    PixGeom g;
    const bool live = stage_pixel(g, p0, s);
    const int lane = tid & 63, wv = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    f32x4 c[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) c[m][0] = c[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < Q; q0 += kSemQ) {
        const int nq = min(kSemQ, Q - q0);
        __syncthreads();
        stage_sigmoids<kTtaSigRow>(sig, masks, s.stride_q, g, live, q0, nq);
        stage_probs<KC, PR>(pr, probs, K, cbase, q0, nq);
        __syncthreads();
        const int ksteps = (nq + 3) >> 2;                    // rows nq .. kSemQ - 1 are staged as zeros
        for (int ks = 0; ks < ksteps; ++ks) {
            const int kr = ks * 4 + lk;
            const float b0 = sig[kr * kTtaSigRow + wv * 32 + lr];
            const float b1 = sig[kr * kTtaSigRow + wv * 32 + 16 + lr];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float a = pr[kr * PR + m * 16 + lr];
                c[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, c[m][0], 0, 0, 0);
                c[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, c[m][1], 0, 0, 0);
            }
        }
    }
    float* stg = sig + wv * (16 * kTtaOutRow);               // one region per wave
    __syncthreads();                                         // every wave has left the product: sig is free
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) stg[(4 * lk + r) * kTtaOutRow + n * 16 + lr] = c[m][n][r];
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = lane + 64 * j;
            const int cl = idx >> 3, pg = idx & 7;
            const int cc = cbase + m * 16 + cl;
            const int64_t px = p0 + wv * 32 + pg * 4;
            if (cc < K && px < HW)
                tta_put4(acc + (int64_t)cc * HW, px, HW, W, mode, vec != 0, *(const float4*)(stg + cl * kTtaOutRow + pg * 4));
        }
    }
}

// "after" mode: thread = four consecutive output pixels, blockIdx.y = a chunk of kTtaResC classes; the taps are computed once and
// every plane of the chunk is resized with them (tap() / lerp2: the roundings of F.interpolate, no contraction)
constexpr int kTtaResC = 16;
__global__ __launch_bounds__(kT) void seg_tta_resize_add_kernel(const float* __restrict__ scores, int K, int hi, int wi, int H, int W,
                                                                int mode, int vec, float* __restrict__ acc)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t px = ((int64_t)blockIdx.x * kT + threadIdx.x) * 4;
    if (px >= HW) return;
    int o[4][4];
    float wy[4][2], wx[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = min(px + i, HW - 1);
        const Tap ty = tap((int)(p / W), hi, H), tx = tap((int)(p % W), wi, W);
        o[i][0] = ty.i0 * wi + tx.i0; o[i][1] = ty.i0 * wi + tx.i1;
        o[i][2] = ty.i1 * wi + tx.i0; o[i][3] = ty.i1 * wi + tx.i1;
        wy[i][0] = ty.l0; wy[i][1] = ty.l1;
        wx[i][0] = tx.l0; wx[i][1] = tx.l1;
    }
    const int64_t plane = (int64_t)hi * wi;
    const int c1 = min(K, ((int)blockIdx.y + 1) * kTtaResC);
    for (int cc = blockIdx.y * kTtaResC; cc < c1; ++cc) {
        const float* s = scores + cc * plane;
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = lerp2(wy[i][0], wy[i][1], wx[i][0], wx[i][1], s[o[i][0]], s[o[i][1]], s[o[i][2]], s[o[i][3]]);
        tta_put4(acc + (int64_t)cc * HW, px, HW, W, mode, vec != 0, make_float4(e[0], e[1], e[2], e[3]));
    }
}

// labels == NULL: acc[i] /= count over the n = K * H * W sums (vec: n is a multiple of 4 and acc 16-byte aligned).  Otherwise thread
// = pixel: labels[p] = argmax_c(acc[c][p] / count), classes ascending with a strict ">" (the lowest class wins a tie): the argmax of
// exactly the values the other form writes
__global__ __launch_bounds__(kT) void seg_tta_finish_kernel(float* __restrict__ acc, int K, int64_t HW, float count, int vec,
                                                            int* __restrict__ labels)
{
    const int64_t t0 = (int64_t)blockIdx.x * kT + threadIdx.x, step = (int64_t)gridDim.x * kT;
    if (labels) {
        for (int64_t p = t0; p < HW; p += step) {
            float best = -INFINITY;
            int bi = 0;
            for (int cc = 0; cc < K; ++cc) {
                const float v = __fdiv_rn(acc[cc * HW + p], count);
                if (v > best) { best = v; bi = cc; }
            }
            labels[p] = bi;
        }
        return;
    }
    const int64_t n = (int64_t)K * HW;
    if (vec) {
        float4* a4 = (float4*)acc;
        for (int64_t i = t0; i < n / 4; i += step) {
            const float4 v = a4[i];
            a4[i] = make_float4(__fdiv_rn(v.x, count), __fdiv_rn(v.y, count), __fdiv_rn(v.z, count), __fdiv_rn(v.w, count));
        }
    } else {
        for (int64_t i = t0; i < n; i += step) acc[i] = __fdiv_rn(acc[i], count);
    }
}

// ---- host side: argument checks and launches that several entry points share -------------------------------------------------------
// the entries of an instance route are blockIdx.y of its kernels
int check_entries(const char* who, int T)
{
    return T <= 0 || T > 65535 ? fail_who(MPF_E_SHAPE, who, "need 1 <= T <= 65535 entries") : 0;
}

int check_tta_mode(const char* who, int mode)
{
    if (!(mode & ~3)) return 0;
    char what[96];
    snprintf(what, sizeof what, "mode has bit 0 (add) and bit 1 (hflip) only, got %d", mode);
    return fail_who(MPF_E_SHAPE, who, what);
}

// the float4 form of tta_put4: whole rows of four (mirrored: W itself) and 16-byte aligned planes
int tta_vec(const float* acc, int H, int W, int mode)
{
    const int64_t HW = (int64_t)H * W;
    return ((uintptr_t)acc & 15) == 0 && (HW & 3) == 0 && (!(mode & 2) || (W & 3) == 0);
}

// f(std::integral_constant<int, V>) for the V among Vs that equals v: a run-time tile count to a template argument
template <int... Vs, typename F>
void with_int(int v, F&& f)
{
    (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// seg_product: labels != NULL -> the argmax epilogue, else the scores stored to out
void launch_product(const void* masks, int dtype, const SegGeom& g, const float* probs, int K, float* out, int* labels, hipStream_t st)
{
    const unsigned tiles = (unsigned)ceil_div((int64_t)g.H * g.W, kSemPix);
    with_mask_type(dtype, masks, [&](auto* m) {
        using T = elem_t<decltype(m)>;
        // classes per thread: chunks of 8 * C = 32, 64, 96 or 192 classes (K > 192: several chunks, on blockIdx.y or in the argmax loop)
        with_int<4, 8, 12, 24>(K <= 32 ? 4 : K <= 64 ? 8 : K <= 96 ? 12 : 24, [&](auto cpt) {
            constexpr int C = decltype(cpt)::value;
            if (labels)
                hipLaunchKernelGGL((seg_labels_kernel<T, C>), dim3(tiles), dim3(kT), 0, st, m, g, probs, K, labels);
            else
                hipLaunchKernelGGL((seg_semantic_kernel<T, C>), dim3(tiles, (unsigned)ceil_div(K, 8 * C)), dim3(kT), 0, st, m, g, probs, K, out);
        });
    });
}

// seg_instance_kernel over T entries: the partial sums of their scores (masks_out NULL) or their 0/1 masks
void launch_instance(const void* masks, int dtype, const SegGeom& g, const int64_t* sel_q, int T, float* masks_out, float2* partial,
                     hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div((int64_t)g.H * g.W, kInstPix), (unsigned)T);
    with_mask_type(dtype, masks, [&](auto* m) {
        hipLaunchKernelGGL(seg_instance_kernel<elem_t<decltype(m)>>, grid, dim3(kT), 0, st, m, g, sel_q, masks_out, partial);
    });
}

// seg_rle_bits_kernel over T entries into bits [T, nwords]
void launch_rle_bits(const void* masks, int dtype, const SegGeom& g, const int64_t* sel_q, int T, int64_t nwords, unsigned long long* bits,
                     hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div((int64_t)g.H * g.W, kInstPix), (unsigned)T);
    with_mask_type(dtype, masks, [&](auto* m) {
        hipLaunchKernelGGL(seg_rle_bits_kernel<elem_t<decltype(m)>>, grid, dim3(kT), 0, st, m, g, sel_q, nwords, bits);
    });
}

}  // namespace

extern "C" int mpf_seg_softmax(const float* cls, int Q, int K1, float object_mask_threshold, float* probs, float* max_score,
                               int* max_label, int* kept, float* kept_score, void* stream)
{
    if (!cls || !probs || !max_score || !max_label || !kept || !kept_score) return mpf::fail(MPF_E_NULL, "seg_softmax: NULL buffer");
    if (Q <= 0 || Q > kMaxQ || K1 < 2) return mpf::fail(MPF_E_SHAPE, "seg_softmax: need 1 <= Q <= 1024 queries and K + 1 >= 2 columns");
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_softmax_kernel");
    hipLaunchKernelGGL(seg_softmax_kernel, dim3(1), dim3(kT), 0, st, cls, Q, K1, object_mask_threshold, probs, max_score, max_label, kept,
                       kept_score);
    mpf::prof_end("seg_softmax_kernel", st, 8.0 * Q * K1);
    return mpf::check(hipGetLastError(), "mpf_seg_softmax");
}

extern "C" int mpf_seg_semantic(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi, int wi,
                                int H, int W, const float* probs, int K, float* out, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_semantic", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!probs || !out) return mpf::fail(MPF_E_NULL, "seg_semantic: NULL buffer");
    if (K <= 0) return mpf::fail(MPF_E_SHAPE, "seg_semantic: K must be positive");
    const int64_t HW = (int64_t)H * W;
    if (K * HW >= (1ll << 40)) return mpf::fail(MPF_E_TOO_LARGE, "seg_semantic: output too large");
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_semantic_kernel");
    launch_product(masks, dtype, g, probs, K, out, nullptr, st);
    mpf::prof_end("seg_semantic_kernel", st, logit_bytes(Q, g, dtype) + 4.0 * K * HW, 2.0 * K * Q * (double)HW);
    return mpf::check(hipGetLastError(), "mpf_seg_semantic");
}

extern "C" size_t mpf_seg_instance_workspace_bytes(int T, int H, int W)
{
    if (T <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)(T * ceil_div((int64_t)H * W, kInstPix)) * sizeof(float2);
}

extern "C" int mpf_seg_instance_scores(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi,
                                       int wi, int H, int W, const int64_t* sel_q, const float* cls_score, int T, float* scores,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_instance_scores", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!sel_q || !cls_score || !scores || !workspace) return mpf::fail(MPF_E_NULL, "seg_instance_scores: NULL buffer");
    if (int e = check_entries("seg_instance_scores", T)) return e;
    if (workspace_bytes < mpf_seg_instance_workspace_bytes(T, H, W)) return mpf::fail(MPF_E_SHAPE, "seg_instance_scores: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (int)ceil_div((int64_t)H * W, kInstPix);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_instance_kernel+seg_instance_reduce_kernel");
    launch_instance(masks, dtype, g, sel_q, T, nullptr, (float2*)workspace, st);
    hipLaunchKernelGGL(seg_instance_reduce_kernel, dim3((unsigned)ceil_div(T, kT / 64)), dim3(kT), 0, st, (const float2*)workspace, tiles, T,
                       cls_score, scores);
    mpf::prof_end("seg_instance_scores", st, logit_bytes(T, g, dtype) + 8.0 * T * tiles);
    return mpf::check(hipGetLastError(), "mpf_seg_instance_scores");
}

extern "C" int mpf_seg_instance_masks(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi,
                                      int wi, int H, int W, const int64_t* sel_q, int T, float* masks_out, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_instance_masks", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!sel_q || !masks_out) return mpf::fail(MPF_E_NULL, "seg_instance_masks: NULL buffer");
    if (int e = check_entries("seg_instance_masks", T)) return e;
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_instance_kernel");
    launch_instance(masks, dtype, g, sel_q, T, masks_out, nullptr, st);
    mpf::prof_end("seg_instance_kernel", st, logit_bytes(T, g, dtype) + 4.0 * T * H * W);
    return mpf::check(hipGetLastError(), "mpf_seg_instance_masks");
}

extern "C" int mpf_seg_panoptic_areas(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi,
                                      int wi, int H, int W, const int* kept, const float* kept_score, int* code, int* areas,
                                      void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_panoptic_areas", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!kept || !kept_score || !code || !areas) return mpf::fail(MPF_E_NULL, "seg_panoptic_areas: NULL buffer");
    if (Q > kMaxQ) return mpf::fail(MPF_E_SHAPE, "seg_panoptic_areas: at most 1024 queries");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    if (int e = mpf::check(hipMemsetAsync(areas, 0, 3 * (size_t)Q * sizeof(int), st), "seg_panoptic_areas: memset")) return e;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_panoptic_kernel");
    with_mask_type(dtype, masks, [&](auto* m) {
        hipLaunchKernelGGL(seg_panoptic_kernel<elem_t<decltype(m)>>, dim3((unsigned)ceil_div(HW, kT)), dim3(kT), 0, st, m, g, kept, kept_score,
                           code, areas);
    });
    mpf::prof_end("seg_panoptic_kernel", st, logit_bytes(Q, g, dtype) + 4.0 * HW);
    return mpf::check(hipGetLastError(), "mpf_seg_panoptic_areas");
}

extern "C" int mpf_seg_panoptic_paint(const int* code, int H, int W, const int* lut, int* out, void* stream)
{
    if (!code || !lut || !out) return mpf::fail(MPF_E_NULL, "seg_panoptic_paint: NULL buffer");
    if (H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_panoptic_paint: bad sizes");
    if ((int64_t)H * W >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_panoptic_paint: output too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_paint_kernel");
    hipLaunchKernelGGL(seg_paint_kernel, dim3((unsigned)ceil_div(HW, kT)), dim3(kT), 0, st, code, HW, lut, out);
    mpf::prof_end("seg_paint_kernel", st, 8.0 * HW);
    return mpf::check(hipGetLastError(), "mpf_seg_panoptic_paint");
}

extern "C" int mpf_seg_semantic_labels(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi, int wi,
                                       int H, int W, const float* probs, int K, int* labels, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_semantic_labels", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!probs || !labels) return mpf::fail(MPF_E_NULL, "seg_semantic_labels: NULL buffer");
    if (K <= 0) return mpf::fail(MPF_E_SHAPE, "seg_semantic_labels: K must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_labels_kernel");
    launch_product(masks, dtype, g, probs, K, nullptr, labels, st);
    mpf::prof_end("seg_labels_kernel", st, logit_bytes(Q, g, dtype) + 4.0 * HW, 2.0 * K * Q * (double)HW);
    return mpf::check(hipGetLastError(), "mpf_seg_semantic_labels");
}

extern "C" int mpf_seg_labels_resize(const float* scores, int K, int hi, int wi, int H, int W, int* labels, void* stream)
{
    if (!scores || !labels) return mpf::fail(MPF_E_NULL, "seg_labels_resize: NULL buffer");
    if (K <= 0 || hi <= 0 || wi <= 0 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_labels_resize: bad sizes");
    if ((int64_t)H * W >= (1ll << 31) || (int64_t)K * hi * wi >= (1ll << 40)) return mpf::fail(MPF_E_TOO_LARGE, "seg_labels_resize: too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_labels_resize_kernel");
    hipLaunchKernelGGL(seg_labels_resize_kernel, dim3((unsigned)((HW + kT - 1) / kT)), dim3(kT), 0, st, scores, K, hi, wi, H, W, labels);
    mpf::prof_end("seg_labels_resize_kernel", st, 4.0 * K * hi * wi + 4.0 * HW);
    return mpf::check(hipGetLastError(), "mpf_seg_labels_resize");
}

extern "C" int mpf_seg_tta_accumulate(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi, int wi,
                                      int H, int W, const float* probs, int K, int mode, float* acc, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_tta_accumulate", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!probs || !acc) return mpf::fail(MPF_E_NULL, "seg_tta_accumulate: NULL buffer");
    if (K <= 0) return mpf::fail(MPF_E_SHAPE, "seg_tta_accumulate: K must be positive");
    if (int e = check_tta_mode("seg_tta_accumulate", mode)) return e;
    if ((int64_t)K * H * W >= (1ll << 40)) return mpf::fail(MPF_E_TOO_LARGE, "seg_tta_accumulate: output too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    // class tiles of 16 per workgroup: ADE20K's 150 classes take 10 (160), larger sets chunks of 12 (192) on blockIdx.y
    const int mt = K <= 32 ? 2 : K <= 64 ? 4 : K <= 128 ? 8 : K <= 160 ? 10 : 12;
    const dim3 grid((unsigned)ceil_div(HW, kSemPix), (unsigned)ceil_div(K, 16 * mt));
    const int vec = tta_vec(acc, H, W, mode);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_tta_accumulate_kernel");
    with_mask_type(dtype, masks, [&](auto* m) {
        with_int<2, 4, 8, 10, 12>(mt, [&](auto tiles) {
            hipLaunchKernelGGL((seg_tta_accumulate_kernel<elem_t<decltype(m)>, decltype(tiles)::value>), grid, dim3(kT), 0, st, m, g, probs, K,
                               mode, vec, acc);
        });
    });
    mpf::prof_end("seg_tta_accumulate_kernel", st, logit_bytes(Q, g, dtype) + ((mode & 1) ? 8.0 : 4.0) * K * HW, 2.0 * K * Q * (double)HW);
    return mpf::check(hipGetLastError(), "mpf_seg_tta_accumulate");
}

extern "C" int mpf_seg_tta_resize_add(const float* scores, int K, int hi, int wi, int H, int W, int mode, float* acc, void* stream)
{
    if (!scores || !acc) return mpf::fail(MPF_E_NULL, "seg_tta_resize_add: NULL buffer");
    if (K <= 0 || hi <= 0 || wi <= 0 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_tta_resize_add: bad sizes");
    if (int e = check_tta_mode("seg_tta_resize_add", mode)) return e;
    if ((int64_t)H * W >= (1ll << 31) || (int64_t)hi * wi >= (1ll << 31) || (int64_t)K * H * W >= (1ll << 40) ||
        (int64_t)K * hi * wi >= (1ll << 40))
        return mpf::fail(MPF_E_TOO_LARGE, "seg_tta_resize_add: too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)(((HW + 3) / 4 + kT - 1) / kT), (unsigned)((K + kTtaResC - 1) / kTtaResC));
    mpf::prof_begin(st);
    mpf::set_kernel("seg_tta_resize_add_kernel");
    hipLaunchKernelGGL(seg_tta_resize_add_kernel, grid, dim3(kT), 0, st, scores, K, hi, wi, H, W, mode, tta_vec(acc, H, W, mode), acc);
    mpf::prof_end("seg_tta_resize_add_kernel", st, 4.0 * K * hi * wi + ((mode & 1) ? 8.0 : 4.0) * K * HW, 14.0 * K * (double)HW);
    return mpf::check(hipGetLastError(), "mpf_seg_tta_resize_add");
}

extern "C" int mpf_seg_tta_finish(float* acc, int K, int H, int W, int count, int* labels, void* stream)
{
    if (!acc) return mpf::fail(MPF_E_NULL, "seg_tta_finish: NULL accumulator");
    if (K <= 0 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_tta_finish: bad sizes");
    if (count <= 0) return mpf::fail(MPF_E_SHAPE, "seg_tta_finish: count must be positive (no view was added)");
    if ((int64_t)H * W >= (1ll << 31) || (int64_t)K * H * W >= (1ll << 40)) return mpf::fail(MPF_E_TOO_LARGE, "seg_tta_finish: too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, n = (int64_t)K * HW;
    const int vec = ((uintptr_t)acc & 15) == 0 && (n & 3) == 0;
    const int64_t units = labels ? HW : vec ? n / 4 : n;
    const unsigned grid = (unsigned)std::min<int64_t>((units + kT - 1) / kT, 64 * (int64_t)mpf::cu_count());
    mpf::prof_begin(st);
    mpf::set_kernel("seg_tta_finish_kernel");
    hipLaunchKernelGGL(seg_tta_finish_kernel, dim3(grid), dim3(kT), 0, st, acc, K, HW, (float)count, vec, labels);
    mpf::prof_end("seg_tta_finish_kernel", st, labels ? 4.0 * n + 4.0 * HW : 8.0 * n, (double)n);
    return mpf::check(hipGetLastError(), "mpf_seg_tta_finish");
}

extern "C" int mpf_seg_confusion_add(const int* pred, const int* gt, int64_t n, int K, int ignore_label, int64_t* conf, void* stream)
{
    if (!pred || !gt || !conf) return mpf::fail(MPF_E_NULL, "seg_confusion_add: NULL buffer");
    if (n <= 0 || K <= 0 || K > 32766) return mpf::fail(MPF_E_SHAPE, "seg_confusion_add: need n > 0 pixels and 1 <= K <= 32766 classes");
    if (n >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_confusion_add: too many pixels for one call");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(K + 1) * (K + 1) * sizeof(int);
    const int64_t nruns = (n + kConfRun - 1) / kConfRun;
    const int64_t want = (nruns + kConfT - 1) / kConfT;
    const bool use_lds = lds <= kConfLdsMax;
    // LDS form: at most one workgroup per CU (every workgroup pays a zero and a flush pass over the histogram)
    const unsigned grid = (unsigned)std::min<int64_t>(want, use_lds ? mpf::cu_count() : 4 * mpf::cu_count());
    unsigned long long* out = (unsigned long long*)conf;
    mpf::prof_begin(st);
    mpf::set_kernel(use_lds ? "seg_confusion_kernel<lds>" : "seg_confusion_kernel<global>");
    if (use_lds) {
        static mpf::LdsAttr attr;
        if (int e = mpf::ensure_dynamic_lds((const void*)seg_confusion_kernel<true>, kConfLdsMax, attr)) return e;
        hipLaunchKernelGGL(seg_confusion_kernel<true>, dim3(grid), dim3(kConfT), lds, st, pred, gt, n, K, ignore_label, out);
    } else {
        hipLaunchKernelGGL(seg_confusion_kernel<false>, dim3(grid), dim3(kConfT), 0, st, pred, gt, n, K, ignore_label, out);
    }
    mpf::prof_end("seg_confusion_kernel", st, 8.0 * n);
    return mpf::check(hipGetLastError(), "mpf_seg_confusion_add");
}

namespace {
struct RleLayout {
    int64_t nwords, tiles;
    size_t bits, tile_off, tile_cnt, total;                  // byte offsets of the three parts, and the size
};
RleLayout rle_layout(int T, int H, int W)
{
    RleLayout l;
    l.nwords = ((int64_t)H * W + 63) / 64;
    l.tiles = (l.nwords + kRleWords - 1) / kRleWords;
    l.bits = 0;
    l.tile_off = (size_t)T * l.nwords * 8;
    l.tile_cnt = l.tile_off + (size_t)T * l.tiles * 8;
    l.total = l.tile_cnt + (((size_t)T * l.tiles * 4 + 7) & ~(size_t)7);
    return l;
}
}  // namespace

extern "C" size_t mpf_seg_instance_rle_workspace_bytes(int T, int H, int W)
{
    if (T <= 0 || H <= 0 || W <= 0) return 0;
    return rle_layout(T, H, W).total;
}

extern "C" int mpf_seg_instance_rle_count(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi,
                                          int wi, int H, int W, const int64_t* sel_q, int T, int64_t* offsets, void* workspace,
                                          size_t workspace_bytes, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_instance_rle_count", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!sel_q || !offsets || !workspace) return mpf::fail(MPF_E_NULL, "seg_instance_rle_count: NULL buffer");
    if (int e = check_entries("seg_instance_rle_count", T)) return e;
    const RleLayout l = rle_layout(T, H, W);
    if (workspace_bytes < l.total) return mpf::fail(MPF_E_SHAPE, "seg_instance_rle_count: workspace too small");
    if (((uintptr_t)workspace & 7) != 0) return mpf::fail(MPF_E_SHAPE, "seg_instance_rle_count: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    char* ws = (char*)workspace;
    unsigned long long* bits = (unsigned long long*)(ws + l.bits);
    int64_t* tile_off = (int64_t*)(ws + l.tile_off);
    int* tile_cnt = (int*)(ws + l.tile_cnt);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_bits_kernel+seg_rle_count_kernel+seg_rle_scan_kernel");
    launch_rle_bits(masks, dtype, g, sel_q, T, l.nwords, bits, st);
    launch_rle_count_scan(bits, T, l.nwords, l.tiles, HW, tile_cnt, tile_off, offsets, st);
    mpf::prof_end("seg_rle_bits_kernel", st, logit_bytes(T, g, dtype) + (double)T * HW / 8);
    return mpf::check(hipGetLastError(), "mpf_seg_instance_rle_count");
}

// the packed words of seg_rle_bits_kernel alone, into the caller's [T, nwords] buffer (the prediction side of csrc/seg_ap.hip)
extern "C" int mpf_seg_instance_bits(const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi, int wi,
                                     int H, int W, const int64_t* sel_q, int T, uint64_t* bits, void* stream)
{
    SegGeom g;
    if (int e = check_geom("seg_instance_bits", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (!sel_q || !bits) return mpf::fail(MPF_E_NULL, "seg_instance_bits: NULL buffer");
    if (int e = check_entries("seg_instance_bits", T)) return e;
    if (((uintptr_t)bits & 7) != 0) return mpf::fail(MPF_E_SHAPE, "seg_instance_bits: bits must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_bits_kernel");
    launch_rle_bits(masks, dtype, g, sel_q, T, ceil_div(HW, 64), (unsigned long long*)bits, st);
    mpf::prof_end("seg_rle_bits_kernel", st, logit_bytes(T, g, dtype) + (double)T * HW / 8);
    return mpf::check(hipGetLastError(), "mpf_seg_instance_bits");
}

extern "C" int mpf_seg_instance_rle_write(const void* workspace, size_t workspace_bytes, int T, int H, int W, const int64_t* offsets,
                                          int64_t total, uint32_t* pos, uint32_t* counts, void* stream)
{
    if (!workspace || !offsets || !pos || !counts) return mpf::fail(MPF_E_NULL, "seg_instance_rle_write: NULL buffer");
    if (T <= 0 || T > 65535 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_instance_rle_write: bad sizes");
    if ((int64_t)H * W >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_instance_rle_write: output too large");
    // every entry has at least its end mark and at most one boundary per position
    if (total < T || total > (int64_t)T * ((int64_t)H * W + 1)) return mpf::fail(MPF_E_SHAPE, "seg_instance_rle_write: total is not offsets[T]");
    const RleLayout l = rle_layout(T, H, W);
    if (workspace_bytes < l.total) return mpf::fail(MPF_E_SHAPE, "seg_instance_rle_write: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    const char* ws = (const char*)workspace;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_scatter_kernel+seg_rle_diff_kernel");
    launch_rle_write((const unsigned long long*)(ws + l.bits), T, l.nwords, l.tiles, HW, (const int64_t*)(ws + l.tile_off), offsets, total, pos,
                     counts, st);
    mpf::prof_end("seg_rle_scatter_kernel", st, (double)T * HW / 8 + 12.0 * total);
    return mpf::check(hipGetLastError(), "mpf_seg_instance_rle_write");
}
