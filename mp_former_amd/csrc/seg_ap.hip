// Instance mask AP on the device for MI355X: mask IoU and the per-image matching of the COCO evaluation, as the reference carries it
// in mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py (evaluateVid, :267-345; an image is a one-frame video), without a
// dense mask leaving the device.
//
// Masks are packed bits in the layout seg_rle_bits_kernel (seg_infer.hip) writes: position p = x * H + y (column-major), 64 positions
// per uint64 word, bit b of word j = position 64 j + b, bits at or past H * W zero.
//
//   seg_pack_masks_kernel    dense [M, H, W] (uint8 / bool bytes or fp32, non-zero = set) -> packed words: one wave ballot per word
//   seg_mask_pairs_kernel    inter[t][g] = popcount(a_t & b_g), area_a[t], area_b[g]: a workgroup stages kPairWords words of up to
//                            kPairRows masks of each side in LDS (word-major, so a wave's lanes read consecutive 8-byte slots), every
//                            thread walks (t, g) pairs over the tile and flushes the non-zero partial counts with integer atomics
//   seg_ap_records_kernel    one thread per detection: score bits, category, rank inside (image, category), image index; the two bit
//                            words zero
//   seg_ap_match_kernel      one thread per (category, area range, IoU threshold): the loop of evaluateVid over the category's first
//                            maxDet detections and its ground truths, non-ignored first; sets the "matched" / "ignored" bit of its
//                            setting in the detections' records and adds the non-ignored ground truths to npig[k][a].
//                            The loop exists once; where a pair's IoU comes from is its template parameter:
//                            <ApCounts> reads the mask counts alone.  dt_area != NULL (mpf_seg_ap_match_tube): a video.  The counts are
//                            those of tubes (the frames' packed words concatenated: popcount(a & b) is the tube intersection, area_a +
//                            area_b - inter iou_seq's union, :203-217) and the ranges test avg_area on both sides (:283, :330).
//                            <ApBoundary> (mpf_seg_ap_match_boundary): a second set of counts, those of the masks' boundaries
//                            (seg_boundary.hip), and a pair's IoU is the smaller of the two (boundary-iou-api's computeBoundaryIoU,
//                            which the reference's tools/evaluate_coco_boundary_ap.py runs).
//                            <ApBoxes> (mpf_seg_ap_match_box): XYWH float64 boxes and pycocotools' bbIou, the "bbox" task of COCO
//                            (boxes of packed masks: seg_box.hip)
//
// Exactness: counts are integers; iou = (double)inter / (double)union is the correctly rounded quotient of two integers below 2^53, as
// python's float / float of the same integers is; the thresholds are the float64 values the host computed (np.linspace), uploaded as
// they are and only compared.  No float atomics, no workgroup waits on another: ordering comes from the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mpf_common.h"

namespace {

constexpr int kApT = 256;
constexpr int kPairRows = 128;     // masks of one side per workgroup
constexpr int kPairWords = 32;     // words per tile: 2 * 128 * 32 * 8 B = 64 KiB of LDS (two workgroups per CU, well under 160 KiB)

template <typename T>
__global__ __launch_bounds__(kApT) void seg_pack_masks_kernel(const T* __restrict__ masks, int H, int W, int64_t nwords,
                                                              unsigned long long* __restrict__ bits)
{
    const int m = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kApT + threadIdx.x;        // wave-aligned: a wave covers one word
    bool on = false;
    if (p < HW) {
        const int y = (int)(p % H), x = (int)(p / H);
        on = masks[(int64_t)m * HW + (int64_t)y * W + x] != (T)0;
    }
    const unsigned long long b = __ballot(on);
    if ((threadIdx.x & 63) == 0 && (p >> 6) < nwords) bits[(int64_t)m * nwords + (p >> 6)] = b;
}

__global__ __launch_bounds__(kApT) void seg_mask_pairs_kernel(const unsigned long long* __restrict__ a, int T,
                                                              const unsigned long long* __restrict__ b, int G, int64_t nwords,
                                                              int* __restrict__ inter, int* __restrict__ area_a,
                                                              int* __restrict__ area_b)
{
    __shared__ unsigned long long la[kPairWords * kPairRows];          // [word][mask]
    __shared__ unsigned long long lb[kPairWords * kPairRows];
    const int64_t w0 = (int64_t)blockIdx.x * kPairWords;
    const int nw = (int)min((int64_t)kPairWords, nwords - w0);
    const int t0 = blockIdx.y * kPairRows, g0 = blockIdx.z * kPairRows;
    const int tc = min(kPairRows, T - t0), gc = min(kPairRows, G - g0);
    for (int i = threadIdx.x; i < tc * kPairWords; i += kApT) {
        const int r = i / kPairWords, w = i % kPairWords;
        la[w * kPairRows + r] = w < nw ? a[(int64_t)(t0 + r) * nwords + w0 + w] : 0ull;
    }
    for (int i = threadIdx.x; i < gc * kPairWords; i += kApT) {
        const int r = i / kPairWords, w = i % kPairWords;
        lb[w * kPairRows + r] = w < nw ? b[(int64_t)(g0 + r) * nwords + w0 + w] : 0ull;
    }
    __syncthreads();
    if (blockIdx.z == 0)
        for (int r = threadIdx.x; r < tc; r += kApT) {
            int c = 0;
            for (int w = 0; w < nw; ++w) c += __popcll(la[w * kPairRows + r]);
            if (c) atomicAdd(&area_a[t0 + r], c);
        }
    if (blockIdx.y == 0)
        for (int r = threadIdx.x; r < gc; r += kApT) {
            int c = 0;
            for (int w = 0; w < nw; ++w) c += __popcll(lb[w * kPairRows + r]);
            if (c) atomicAdd(&area_b[g0 + r], c);
        }
    for (int i = threadIdx.x; i < tc * gc; i += kApT) {
        const int t = i / gc, g = i % gc;              // a wave's lanes: consecutive g (consecutive LDS slots), at most two t (broadcast)
        int c = 0;
        for (int w = 0; w < nw; ++w) c += __popcll(la[w * kPairRows + t] & lb[w * kPairRows + g]);
        if (c) atomicAdd(&inter[(int64_t)(t0 + t) * G + g0 + g], c);
    }
}

// record of one detection: 4 x int64 = {score bits | category << 32, rank | image << 32, matched bits, ignored bits}
constexpr int kApRec = 4;

__global__ __launch_bounds__(kApT) void seg_ap_records_kernel(const float* __restrict__ dt_score, const int* __restrict__ dt_cat, int D,
                                                              int image, unsigned long long* __restrict__ rec)
{
    const int d = blockIdx.x * kApT + threadIdx.x;
    if (d >= D) return;
    const int c = dt_cat[d];
    int rank = 0;
    for (int e = 0; e < d; ++e) rank += dt_cat[e] == c;
    rec[(int64_t)kApRec * d + 0] = (unsigned long long)__float_as_uint(dt_score[d]) | ((unsigned long long)(unsigned)c << 32);
    rec[(int64_t)kApRec * d + 1] = (unsigned long long)(unsigned)rank | ((unsigned long long)(unsigned)image << 32);
    rec[(int64_t)kApRec * d + 2] = 0ull;
    rec[(int64_t)kApRec * d + 3] = 0ull;
}

// crowd_rule 0 = "coco" (pycocotools' rleIou: a crowd ground truth divides by the detection's area), 1 = "union" (the reference
// file's own computeIoU: the plain union for every pair)
__device__ __forceinline__ double ap_iou(int inter, int area_d, int area_g, bool crowd, int crowd_rule)
{
    if (inter == 0) return 0.0;
    const int64_t uni = (crowd && crowd_rule == 0) ? (int64_t)area_d : (int64_t)area_d + (int64_t)area_g - inter;
    return (double)inter / (double)uni;
}

// The IoU sources of seg_ap_match_kernel: iou(d, g, crowd, crowd_rule) of a pair and det_area(d), the area the ranges test for an
// unmatched detection.
// ApCounts: the integer counts of mpf_seg_mask_pairs; dt_area != NULL (tubes): avg_area, not the IoU's pixel count
struct ApCounts {
    const int* __restrict__ inter;
    const int* __restrict__ area_d;
    const int* __restrict__ area_g;
    const double* __restrict__ dt_area;
    int G;
    __device__ __forceinline__ double iou(int d, int g, bool crowd, int crowd_rule) const
    {
        return ap_iou(inter[(int64_t)d * G + g], area_d[d], area_g[g], crowd, crowd_rule);
    }
    __device__ __forceinline__ double det_area(int d) const { return dt_area ? dt_area[d] : (double)area_d[d]; }
};

// ApBoundary: a second set of counts (the masks' boundaries, csrc/seg_boundary.hip) and the pair's IoU is the smaller of the two
// (boundary-iou-api, COCOeval.computeBoundaryIoU); areas and ranges stay the masks'
struct ApBoundary {
    ApCounts mask, bnd;
    __device__ __forceinline__ double iou(int d, int g, bool crowd, int crowd_rule) const
    {
        return fmin(mask.iou(d, g, crowd, crowd_rule), bnd.iou(d, g, crowd, crowd_rule));
    }
    __device__ __forceinline__ double det_area(int d) const { return mask.det_area(d); }
};

// ApBoxes: XYWH float64 boxes and pycocotools' bbIou (maskApi.c) in its operation order.  Every product, sum and quotient is rounded
// on its own: the two bodies are compiled with contraction off (`#pragma clang fp contract(off)`; hipcc's default would fuse
// gw * gh + da and (da + ga) - w * h into v_fma_f64, and the __dmul_rn family of this ROCm's headers are plain operators that fuse
// the same way), so a host restatement in IEEE double gives the same bits and no ">= threshold" decision differs by rounding.  An
// unmatched detection is tested with w * h, the "area" COCO's loadRes gives a bbox result.
struct ApBoxes {
    const double* __restrict__ dt_box;
    const double* __restrict__ gt_box;
    __device__ __forceinline__ double iou(int d, int g, bool crowd, int crowd_rule) const
    {
#pragma clang fp contract(off)
        const double dx = dt_box[4 * (int64_t)d], dy = dt_box[4 * (int64_t)d + 1], dw = dt_box[4 * (int64_t)d + 2], dh = dt_box[4 * (int64_t)d + 3];
        const double gx = gt_box[4 * (int64_t)g], gy = gt_box[4 * (int64_t)g + 1], gw = gt_box[4 * (int64_t)g + 2], gh = gt_box[4 * (int64_t)g + 3];
        const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
        const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        if (w <= 0.0 || h <= 0.0) return 0.0;
        const double i = w * h, da = dw * dh;
        if (crowd && crowd_rule == 0) return i / da;
        const double ga = gw * gh;
        const double s = da + ga;
        const double u = s - i;
        return i / u;
    }
    __device__ __forceinline__ double det_area(int d) const
    {
#pragma clang fp contract(off)
        const double w = dt_box[4 * (int64_t)d + 2], h = dt_box[4 * (int64_t)d + 3];
        return w * h;
    }
};

template <class Iou>
__global__ __launch_bounds__(kApT) void seg_ap_match_kernel(const Iou src, int D, int G, const int* __restrict__ dt_cat,
                                                            const int* __restrict__ gt_cat, const int* __restrict__ gt_crowd,
                                                            const double* __restrict__ gt_area, const double* __restrict__ thrs, int Tn,
                                                            const double* __restrict__ rngs, int A, int K, int max_det, int crowd_rule,
                                                            unsigned long long* __restrict__ rec, long long* __restrict__ npig,
                                                            unsigned char* __restrict__ gtm_all)
{
    const int idx = blockIdx.x * kApT + threadIdx.x;
    if (idx >= K * A * Tn) return;
    const int k = idx / (A * Tn), a = (idx / Tn) % A, ti = idx % Tn;
    const double lo = rngs[2 * a], hi = rngs[2 * a + 1], thr = thrs[ti];
    const unsigned long long bit = 1ull << (a * Tn + ti);
    unsigned char* gtm = gtm_all + (size_t)(a * Tn + ti) * G;          // only this thread touches the entries of category k
    int nonig = 0;
    for (int g = 0; g < G; ++g) {
        if (gt_cat[g] != k) continue;
        gtm[g] = 0;
        const double ga = gt_area[g];
        if (!(gt_crowd[g] || ga < lo || ga > hi)) ++nonig;
    }
    if (ti == 0 && nonig) npig[k * A + a] += nonig;                    // one writer per (k, a); calls are ordered by the stream
    const double start = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
    int taken = 0;
    for (int d = 0; d < D && taken < max_det; ++d) {
        if (dt_cat[d] != k) continue;
        ++taken;
        double best = start;
        int m = -1, m_ig = 0;
        bool stop = false;
        for (int pass = 0; pass < 2 && !stop; ++pass)                   // ground truths with _ignore == 0 first, then _ignore == 1 (:289)
            for (int g = 0; g < G; ++g) {
                if (gt_cat[g] != k) continue;
                const bool crowd = gt_crowd[g] != 0;
                const double ga = gt_area[g];
                const int ig = (crowd || ga < lo || ga > hi) ? 1 : 0;
                if (ig != pass) continue;
                if (gtm[g] && !crowd) continue;                         // :312
                if (m > -1 && m_ig == 0 && ig == 1) { stop = true; break; }     // :315
                const double v = src.iou(d, g, crowd, crowd_rule);
                if (v < best) continue;                                 // :318: equality takes the later ground truth
                best = v;
                m = g;
                m_ig = ig;
            }
        bool ignored;
        if (m >= 0) {
            gtm[m] = 1;
            ignored = m_ig != 0;
            atomicOr(&rec[(int64_t)kApRec * d + 2], bit);
        } else {
            const double da = src.det_area(d);
            ignored = da < lo || da > hi;                               // :330-331
        }
        if (ignored) atomicOr(&rec[(int64_t)kApRec * d + 3], bit);
    }
}

}  // namespace

extern "C" int mpf_seg_pack_masks(const void* masks, int dtype, int M, int H, int W, uint64_t* bits, void* stream)
{
    if (M < 0 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_pack_masks: need M >= 0 masks of H, W > 0");
    if (dtype != MPF_U8 && dtype != MPF_F32) return mpf::fail(MPF_E_DTYPE, "seg_pack_masks: masks must be uint8 / bool bytes or f32 (dtype)");
    if (M == 0) return 0;
    if (!masks || !bits) return mpf::fail(MPF_E_NULL, "seg_pack_masks: NULL buffer");
    if ((int64_t)H * W >= (1ll << 31) || M > 65535) return mpf::fail(MPF_E_TOO_LARGE, "seg_pack_masks: too large (H * W < 2^31, M <= 65535)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = (HW + 63) / 64;
    const dim3 grid((unsigned)((HW + kApT - 1) / kApT), (unsigned)M);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_pack_masks_kernel");
    if (dtype == MPF_U8)
        hipLaunchKernelGGL(seg_pack_masks_kernel<unsigned char>, grid, dim3(kApT), 0, st, (const unsigned char*)masks, H, W, nwords,
                           (unsigned long long*)bits);
    else
        hipLaunchKernelGGL(seg_pack_masks_kernel<float>, grid, dim3(kApT), 0, st, (const float*)masks, H, W, nwords,
                           (unsigned long long*)bits);
    mpf::prof_end("seg_pack_masks_kernel", st, (double)M * HW * (dtype == MPF_U8 ? 1 : 4) + (double)M * nwords * 8);
    return mpf::check(hipGetLastError(), "mpf_seg_pack_masks");
}

extern "C" int mpf_seg_mask_pairs(const uint64_t* a_bits, int T, const uint64_t* b_bits, int G, int64_t nwords, int* inter, int* area_a,
                                  int* area_b, void* stream)
{
    if (T < 0 || G < 0 || nwords <= 0) return mpf::fail(MPF_E_SHAPE, "seg_mask_pairs: need T, G >= 0 masks of nwords > 0 words");
    if (nwords >= (1ll << 25) || (int64_t)T * G >= (1ll << 31) || T > 65535 * kPairRows || G > 65535 * kPairRows)
        return mpf::fail(MPF_E_TOO_LARGE, "seg_mask_pairs: too large");
    if ((T && (!a_bits || !area_a)) || (G && (!b_bits || !area_b)) || (T && G && !inter))
        return mpf::fail(MPF_E_NULL, "seg_mask_pairs: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    // the counters are zeroed here: the kernel adds its non-zero partial counts
    if (T) if (int e = mpf::check(hipMemsetAsync(area_a, 0, sizeof(int) * (size_t)T, st), "mpf_seg_mask_pairs")) return e;
    if (G) if (int e = mpf::check(hipMemsetAsync(area_b, 0, sizeof(int) * (size_t)G, st), "mpf_seg_mask_pairs")) return e;
    if (T && G) if (int e = mpf::check(hipMemsetAsync(inter, 0, sizeof(int) * (size_t)T * G, st), "mpf_seg_mask_pairs")) return e;
    if (T == 0 && G == 0) return 0;
    // one side empty: the other side's areas are still counted (the empty side contributes one chunk without rows)
    const dim3 grid((unsigned)((nwords + kPairWords - 1) / kPairWords), (unsigned)std::max(1, (T + kPairRows - 1) / kPairRows),
                    (unsigned)std::max(1, (G + kPairRows - 1) / kPairRows));
    mpf::prof_begin(st);
    mpf::set_kernel("seg_mask_pairs_kernel");
    hipLaunchKernelGGL(seg_mask_pairs_kernel, grid, dim3(kApT), 0, st, (const unsigned long long*)a_bits, T,
                       (const unsigned long long*)b_bits, G, nwords, inter, area_a, area_b);
    mpf::prof_end("seg_mask_pairs_kernel", st, 8.0 * nwords * ((double)T + G) + 4.0 * T * G);
    return mpf::check(hipGetLastError(), "mpf_seg_mask_pairs");
}

extern "C" size_t mpf_seg_ap_workspace_bytes(int G, int A, int Tn)
{
    if (G < 0 || A <= 0 || Tn <= 0) return 0;
    return (size_t)A * Tn * G;
}

// What a pair's IoU is computed from: the counts of mpf_seg_mask_pairs (inter [D, G], area_d [D], area_g [G]), with the boundaries'
// counts as a second set (boundary), or XYWH boxes (box: dt_box [D, 4], gt_box [G, 4]).  dt_area (tubes, else NULL): the area the
// ranges test for an unmatched detection, where the images' entries take the pixel count area_d
struct ApSource {
    bool boundary = false, box = false;
    const int *inter = nullptr, *area_d = nullptr, *area_g = nullptr, *inter_b = nullptr, *area_db = nullptr, *area_gb = nullptr;
    const double *dt_area = nullptr, *dt_box = nullptr, *gt_box = nullptr;
};

// the body of the four entries: one argument check, one records kernel, one workspace rule, one record format
static int ap_match(const char* where, const ApSource& s, int D, int G, const float* dt_score, const int* dt_cat, const int* gt_cat,
                    const int* gt_crowd, const double* gt_area, const double* iou_thrs, int Tn, const double* area_rngs, int A, int K,
                    int max_det, int crowd_rule, int image, int64_t* records, int64_t* npig, void* workspace, size_t workspace_bytes,
                    void* stream)
{
    if (D < 0 || G < 0 || K <= 0 || A <= 0 || Tn <= 0 || max_det <= 0 || image < 0)
        return mpf::fail(MPF_E_SHAPE, "seg_ap_match: need D, G >= 0, K, A, Tn, max_det > 0 and image >= 0");
    if (A > 64 || Tn > 64 || A * Tn > 64) return mpf::fail(MPF_E_SHAPE, "seg_ap_match: A * Tn > 64 settings do not fit a record's bit words");
    if (crowd_rule != 0 && crowd_rule != 1) return mpf::fail(MPF_E_SHAPE, "seg_ap_match: crowd_rule is 0 (coco) or 1 (union)");
    if ((int64_t)D * G >= (1ll << 31) || (int64_t)K * A * Tn >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_ap_match: too large");
    if (!iou_thrs || !area_rngs || !npig) return mpf::fail(MPF_E_NULL, "seg_ap_match: NULL settings or counters");
    const void* of_d = s.box ? (const void*)s.dt_box : (const void*)s.area_d;
    const void* of_g = s.box ? (const void*)s.gt_box : (const void*)s.area_g;
    if (D && (!of_d || !dt_score || !dt_cat || !records)) return mpf::fail(MPF_E_NULL, "seg_ap_match: NULL detection buffer");
    if (G && (!of_g || !gt_cat || !gt_crowd || !gt_area || !workspace)) return mpf::fail(MPF_E_NULL, "seg_ap_match: NULL ground-truth buffer");
    if (!s.box && D && G && !s.inter) return mpf::fail(MPF_E_NULL, "seg_ap_match: NULL pair counts");
    if (s.boundary && D && G && (!s.inter_b || !s.area_db || !s.area_gb)) return mpf::fail(MPF_E_NULL, "seg_ap_match_boundary: NULL boundary counts");
    if (workspace_bytes < (size_t)A * Tn * G) return mpf::fail(MPF_E_SHAPE, "seg_ap_match: workspace smaller than mpf_seg_ap_workspace_bytes");
    if (D == 0 && G == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    // the launch as mpf_last_kernel reports it; the profiler's name is the part after the records kernel
    static constexpr char kRecordsPlus[] = "seg_ap_records_kernel+";
    const char* launched = s.box ? "seg_ap_records_kernel+seg_ap_match_kernel<box>"
                         : s.boundary ? "seg_ap_records_kernel+seg_ap_match_kernel<boundary>" : "seg_ap_records_kernel+seg_ap_match_kernel";
    const char* name = launched + sizeof(kRecordsPlus) - 1;
    mpf::prof_begin(st);
    mpf::set_kernel(launched);
    if (D)
        hipLaunchKernelGGL(seg_ap_records_kernel, dim3((unsigned)((D + kApT - 1) / kApT)), dim3(kApT), 0, st, dt_score, dt_cat, D, image,
                           (unsigned long long*)records);
    const int n = K * A * Tn;
    const dim3 grid((unsigned)((n + kApT - 1) / kApT));
    auto launch = [&](auto src) {
        hipLaunchKernelGGL(seg_ap_match_kernel<decltype(src)>, grid, dim3(kApT), 0, st, src, D, G, dt_cat, gt_cat, gt_crowd, gt_area, iou_thrs,
                           Tn, area_rngs, A, K, max_det, crowd_rule, (unsigned long long*)records, (long long*)npig,
                           (unsigned char*)workspace);
    };
    const ApCounts mask{s.inter, s.area_d, s.area_g, s.dt_area, G};
    if (s.box)
        launch(ApBoxes{s.dt_box, s.gt_box});
    else if (s.boundary)
        launch(ApBoundary{mask, ApCounts{s.inter_b, s.area_db, s.area_gb, nullptr, G}});
    else
        launch(mask);
    mpf::prof_end(name, st, s.box ? 32.0 * ((double)D + G) + 32.0 * D : (s.boundary ? 8.0 : 4.0) * D * G + 32.0 * D);
    return mpf::check(hipGetLastError(), where);
}

extern "C" int mpf_seg_ap_match(const int* inter, const int* area_d, const int* area_g, int D, int G, const float* dt_score,
                                const int* dt_cat, const int* gt_cat, const int* gt_crowd, const double* gt_area, const double* iou_thrs,
                                int Tn, const double* area_rngs, int A, int K, int max_det, int crowd_rule, int image, int64_t* records,
                                int64_t* npig, void* workspace, size_t workspace_bytes, void* stream)
{
    ApSource s;
    s.inter = inter, s.area_d = area_d, s.area_g = area_g;
    return ap_match("mpf_seg_ap_match", s, D, G, dt_score, dt_cat, gt_cat, gt_crowd, gt_area, iou_thrs, Tn, area_rngs, A, K, max_det,
                    crowd_rule, image, records, npig, workspace, workspace_bytes, stream);
}

// one video: the counts are those of the tubes (the frames' words concatenated), gt_area / dt_area their avg_area (mpf_seg_tube_areas)
extern "C" int mpf_seg_ap_match_tube(const int* inter, const int* area_d, const int* area_g, int D, int G, const float* dt_score,
                                     const int* dt_cat, const int* gt_cat, const int* gt_crowd, const double* gt_area,
                                     const double* dt_area, const double* iou_thrs, int Tn, const double* area_rngs, int A, int K,
                                     int max_det, int crowd_rule, int image, int64_t* records, int64_t* npig, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    if (D > 0 && !dt_area) return mpf::fail(MPF_E_NULL, "seg_ap_match_tube: NULL dt_area");
    ApSource s;
    s.inter = inter, s.area_d = area_d, s.area_g = area_g, s.dt_area = dt_area;
    return ap_match("mpf_seg_ap_match_tube", s, D, G, dt_score, dt_cat, gt_cat, gt_crowd, gt_area, iou_thrs, Tn, area_rngs, A, K, max_det,
                    crowd_rule, image, records, npig, workspace, workspace_bytes, stream);
}

extern "C" int mpf_seg_ap_match_boundary(const int* inter, const int* area_d, const int* area_g, const int* inter_b, const int* area_db,
                                         const int* area_gb, int D, int G, const float* dt_score, const int* dt_cat, const int* gt_cat,
                                         const int* gt_crowd, const double* gt_area, const double* iou_thrs, int Tn,
                                         const double* area_rngs, int A, int K, int max_det, int crowd_rule, int image, int64_t* records,
                                         int64_t* npig, void* workspace, size_t workspace_bytes, void* stream)
{
    ApSource s;
    s.boundary = true;
    s.inter = inter, s.area_d = area_d, s.area_g = area_g, s.inter_b = inter_b, s.area_db = area_db, s.area_gb = area_gb;
    return ap_match("mpf_seg_ap_match_boundary", s, D, G, dt_score, dt_cat, gt_cat, gt_crowd, gt_area, iou_thrs, Tn, area_rngs, A, K,
                    max_det, crowd_rule, image, records, npig, workspace, workspace_bytes, stream);
}

// boxes in place of the counts: XYWH float64, the detections' in score order
extern "C" int mpf_seg_ap_match_box(const double* dt_box, const double* gt_box, int D, int G, const float* dt_score, const int* dt_cat,
                                    const int* gt_cat, const int* gt_crowd, const double* gt_area, const double* iou_thrs, int Tn,
                                    const double* area_rngs, int A, int K, int max_det, int crowd_rule, int image, int64_t* records,
                                    int64_t* npig, void* workspace, size_t workspace_bytes, void* stream)
{
    ApSource s;
    s.box = true;
    s.dt_box = dt_box, s.gt_box = gt_box;
    return ap_match("mpf_seg_ap_match_box", s, D, G, dt_score, dt_cat, gt_cat, gt_crowd, gt_area, iou_thrs, Tn, area_rngs, A, K, max_det,
                    crowd_rule, image, records, npig, workspace, workspace_bytes, stream);
}
