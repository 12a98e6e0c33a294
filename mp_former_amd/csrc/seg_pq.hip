// Panoptic quality (PQ / SQ / RQ) on the device for MI355X: the per-image arithmetic of panopticapi's pq_compute_single_core as the
// reference carries it in tools/evaluate_pq_for_semantic_segmentation.py (pq_compute_single_image, :41-136), without the id map
// leaving the device.
//
//   seg_pq_pairs_kernel   table[gt slot][pred slot] += 1 per pixel (:81-87, the np.unique of gt * OFFSET + pred).  Ids are arbitrary
//                         non-negative int32 values; a slot is: 0 = VOID (id == void_id), 1..G (1..S) = the listed segments in
//                         ascending id order, G+1 (S+1) = neither.  The listed ids are a sorted table (binary search in an LDS copy)
//                         or the contiguous range base .. base+G-1 (direct index).  Built like seg_confusion_kernel: 1024 threads,
//                         8 consecutive pixels per thread with equal neighbours merged (a pixel equal to its left neighbour keeps
//                         its slot), an int32 LDS histogram where the table fits in 128 KiB, flushed with integer atomics on the
//                         non-zero counters, global integer atomics otherwise.  Integers only: the table does not depend on
//                         scheduling.
//   seg_pq_match_kernel   ONE workgroup per image: areas, matches, false negatives, false positives (:89-134) from the table, added
//                         to the running tp / fp / fn int64 [K] and iou float64 [K]; the table is written back to zero.
//
// iou is bit for bit the reference's: every pair's iou = (double)inter / (double)union (python's int / int is the correctly rounded
// quotient, as is the double division of two integers below 2^53); a gt segment has at most one partner with iou > 0.5, so walking
// the gt slots in ascending order IS the reference's ascending (gt id, pred id) order; one thread sums each category's matches of
// the image from 0.0 in that order (PQStat of the single image), then the partial is added to the running total (pq_stat +=
// single).  No float atomics.  Images arrive in stream order and each has one workgroup, so the running totals have one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mpf_common.h"

namespace {

constexpr int kPqT = 1024;         // pair counts: threads per workgroup (16 waves; the histogram is the only LDS user of its CU)
constexpr int kPqRun = 8;          // consecutive pixels per thread
constexpr size_t kPqLdsMax = 128 * 1024;   // as kConfLdsMax of seg_infer.hip: 32 KiB of the CU's 160 KiB stay free
constexpr size_t kPqIdsMax = 64 * 1024;    // the id tables alone (global form) and the match kernel's arrays: the default limit
constexpr int kPqMatchT = 256;

// slot of `id` among n listed ids: ids == nullptr -> the range base .. base + n - 1, else ids[] ascending (LDS copy)
__device__ __forceinline__ int pq_slot(int id, int void_id, const int* ids, int n, int base)
{
    if (id == void_id) return 0;
    if (!ids) {
        const int64_t d = (int64_t)id - base;
        return (d >= 0 && d < n) ? (int)d + 1 : n + 1;
    }
    int lo = 0, hi = n;            // first index with ids[index] >= id
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && ids[lo] == id) ? lo + 1 : n + 1;
}

// RGB: panopticapi's rgb2id, R + 256 G + 65536 B
template <bool RGB>
__device__ __forceinline__ int pq_gt_id(const void* gt, int64_t p)
{
    if (RGB) {
        const unsigned char* b = (const unsigned char*)gt + 3 * p;
        return (int)b[0] | ((int)b[1] << 8) | ((int)b[2] << 16);
    }
    return ((const int*)gt)[p];
}

template <bool LDS, bool RGB>
__global__ __launch_bounds__(kPqT) void seg_pq_pairs_kernel(const int* __restrict__ pred, const void* __restrict__ gt, int64_t n,
                                                            const int* __restrict__ gt_ids, int G, int gt_base,
                                                            const int* __restrict__ pred_ids, int S, int pred_base, int void_id,
                                                            int* __restrict__ table)
{
    extern __shared__ int pq_lds[];            // [gt ids G (if a table)] [pred ids S (if a table)] [histogram (LDS form)]
    const int cols = S + 2;
    const int cells = (G + 2) * cols;
    int* gl = pq_lds;
    int* pl = gl + (gt_ids ? G : 0);
    int* hist = pl + (pred_ids ? S : 0);
    if (gt_ids)
        for (int i = threadIdx.x; i < G; i += kPqT) gl[i] = gt_ids[i];
    if (pred_ids)
        for (int i = threadIdx.x; i < S; i += kPqT) pl[i] = pred_ids[i];
    if (LDS)
        for (int i = threadIdx.x; i < cells; i += kPqT) hist[i] = 0;
    __syncthreads();
    const int* gtab = gt_ids ? gl : nullptr;
    const int* ptab = pred_ids ? pl : nullptr;
    const int64_t nruns = (n + kPqRun - 1) / kPqRun;
    for (int64_t r = (int64_t)blockIdx.x * kPqT + threadIdx.x; r < nruns; r += (int64_t)gridDim.x * kPqT) {
        const int64_t p0 = r * kPqRun;
        const int m = (int)min((int64_t)kPqRun, n - p0);
        int gid = pq_gt_id<RGB>(gt, p0), pid = pred[p0];
        int gs = pq_slot(gid, void_id, gtab, G, gt_base), ps = pq_slot(pid, void_id, ptab, S, pred_base);
        int cur = gs * cols + ps, cnt = 1;
        for (int i = 1; i < m; ++i) {
            const int g2 = pq_gt_id<RGB>(gt, p0 + i), p2 = pred[p0 + i];
            if (g2 == gid && p2 == pid) { ++cnt; continue; }
            if (g2 != gid) { gid = g2; gs = pq_slot(gid, void_id, gtab, G, gt_base); }
            if (p2 != pid) { pid = p2; ps = pq_slot(pid, void_id, ptab, S, pred_base); }
            if (LDS) atomicAdd(&hist[cur], cnt);
            else atomicAdd(&table[cur], cnt);
            cur = gs * cols + ps;
            cnt = 1;
        }
        if (LDS) atomicAdd(&hist[cur], cnt);
        else atomicAdd(&table[cur], cnt);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kPqT) {
            const int v = hist[i];
            if (v) atomicAdd(&table[i], v);
        }
    }
}

// category of listed segment i (the implicit form: the class itself); -1 when the host's table holds a value outside [0, K)
__device__ __forceinline__ int pq_cat(const int* cat, int i, int K)
{
    const int c = cat ? cat[i] : i;
    return (c >= 0 && c < K) ? c : -1;
}

// gt_flags: bit 0 = iscrowd, bit 1 = the crowd segment of its category that comes last in the annotation (:113-119)
constexpr int kPqCrowd = 1, kPqCrowdWins = 2;

__global__ __launch_bounds__(kPqMatchT) void seg_pq_match_kernel(int* __restrict__ table, int G, int S, int K,
                                                                 const int* __restrict__ gt_cat, const int* __restrict__ gt_flags,
                                                                 const int* __restrict__ pred_cat, int implicit,
                                                                 unsigned long long* __restrict__ tp, unsigned long long* __restrict__ fp,
                                                                 unsigned long long* __restrict__ fn, double* __restrict__ iou,
                                                                 unsigned long long* __restrict__ err)
{
    extern __shared__ double pq_match_lds[];
    // doubles first (8-byte aligned): giou [G + 2], part [K]; then ints: rows [G + 2], gmatch [G + 2], colsum [S + 2], pmatch [S + 2],
    // crowd [K]
    double* giou = pq_match_lds;
    double* part = giou + (G + 2);
    int* rowsum = (int*)(part + K);
    int* gmatch = rowsum + (G + 2);
    int* colsum = gmatch + (G + 2);
    int* pmatch = colsum + (S + 2);
    int* crowd = pmatch + (S + 2);
    const int cols = S + 2, rows = G + 2;
    const int cells = rows * cols;
    const int t = threadIdx.x;
    for (int i = t; i < rows; i += kPqMatchT) { rowsum[i] = 0; gmatch[i] = 0; giou[i] = 0.0; }
    for (int i = t; i < cols; i += kPqMatchT) { colsum[i] = 0; pmatch[i] = 0; }
    for (int i = t; i < K; i += kPqMatchT) { crowd[i] = 0; part[i] = 0.0; }
    __syncthreads();
    // areas: pred = column sum (:67-73), gt = row sum (the annotation's "area" of a consistent annotation; :50-56 in the semantic form)
    for (int i = t; i < cells; i += kPqMatchT) {
        const int v = table[i];
        if (v) {
            atomicAdd(&rowsum[i / cols], v);
            atomicAdd(&colsum[i % cols], v);
        }
    }
    if (gt_flags)
        for (int g = 1 + t; g <= G; g += kPqMatchT)
            if ((gt_flags[g - 1] & kPqCrowdWins) && pq_cat(gt_cat, g - 1, K) >= 0) crowd[pq_cat(gt_cat, g - 1, K)] = g;   // one winner per category (host)
    __syncthreads();
    // matches (:92-109): every listed pair with a count, a non-crowd gt and equal categories
    for (int i = t; i < cells; i += kPqMatchT) {
        const int g = i / cols, p = i % cols;
        if (g < 1 || g > G || p < 1 || p > S) continue;
        const int v = table[i];
        if (!v) continue;
        if (gt_flags && (gt_flags[g - 1] & kPqCrowd)) continue;
        if (pq_cat(gt_cat, g - 1, K) != pq_cat(pred_cat, p - 1, K)) continue;
        const int64_t uni = (int64_t)colsum[p] + (int64_t)rowsum[g] - v - table[p];             // table[p] = table[VOID][p]
        const double q = (double)v / (double)uni;
        if (q > 0.5) {                               // at most one partner per gt and per pred: no two threads write one slot
            gmatch[g] = p;
            pmatch[p] = g;
            giou[g] = q;
        }
    }
    __syncthreads();
    // tp and fn (:113-120): a listed gt exists as the annotation lists it (zero pixels included); a class of the semantic form
    // exists where it has pixels
    unsigned long long bad = 0;
    for (int g = 1 + t; g <= G; g += kPqMatchT) {
        if (implicit && rowsum[g] == 0) continue;
        if (gt_flags && (gt_flags[g - 1] & kPqCrowd)) continue;
        const int c = pq_cat(gt_cat, g - 1, K);
        if (c < 0) { ++bad; continue; }
        atomicAdd(gmatch[g] ? &tp[c] : &fn[c], 1ull);
    }
    // fp (:123-134), and what the reference raises KeyError for
    for (int p = 1 + t; p <= S; p += kPqMatchT) {
        const int area = colsum[p];
        if (area == 0) {
            if (!implicit) ++bad;                    // listed, no pixel (:77-78)
            continue;
        }
        if (pmatch[p]) continue;
        const int c = pq_cat(pred_cat, p - 1, K);
        if (c < 0) { ++bad; continue; }               // unknown category (:75-76)
        int64_t inter = table[p];
        if (crowd[c]) inter += table[crowd[c] * cols + p];
        if ((double)inter / (double)area > 0.5) continue;
        atomicAdd(&fp[c], 1ull);
    }
    if (t == 0) {
        bad += (unsigned long long)colsum[S + 1];    // pixels of an id that is not listed (:69-72)
        if (implicit) bad += (unsigned long long)colsum[0];      // the semantic form lists the ignore label as a segment of an unknown category (:59-60, :75-76)
        // the image's iou per category from 0.0, gt slots ascending = (gt id, pred id) ascending
        for (int g = 1; g <= G; ++g)
            if (gmatch[g] && pq_cat(gt_cat, g - 1, K) >= 0) part[pq_cat(gt_cat, g - 1, K)] += giou[g];
    }
    if (bad) atomicAdd(err, bad);
    __syncthreads();
    for (int c = t; c < K; c += kPqMatchT)
        if (part[c] != 0.0) iou[c] += part[c];
    for (int i = t; i < cells; i += kPqMatchT) table[i] = 0;
}

size_t pq_match_lds_bytes(int G, int S, int K)
{
    return sizeof(double) * ((size_t)G + 2 + K) + sizeof(int) * (2 * ((size_t)G + 2) + 2 * ((size_t)S + 2) + K);
}

}  // namespace

extern "C" size_t mpf_seg_pq_workspace_bytes(int G, int S)
{
    if (G < 0 || S < 0) return 0;
    return ((size_t)G + 2) * ((size_t)S + 2) * sizeof(int);
}

extern "C" int mpf_seg_pq_pairs(const int* pred, const void* gt, int gt_format, int64_t n, const int* gt_ids, int G, int gt_base,
                                const int* pred_ids, int S, int pred_base, int void_id, int* table, size_t table_bytes, void* stream)
{
    if (!pred || !gt || !table) return mpf::fail(MPF_E_NULL, "seg_pq_pairs: NULL buffer");
    if (gt_format != 0 && gt_format != 1) return mpf::fail(MPF_E_DTYPE, "seg_pq_pairs: unknown gt format (0 = int32 ids, 1 = uint8 RGB)");
    if (n <= 0 || G < 0 || S < 0) return mpf::fail(MPF_E_SHAPE, "seg_pq_pairs: need n > 0 pixels and G, S >= 0 segments");
    if (n >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_pq_pairs: too many pixels for one call");
    const size_t ids = sizeof(int) * ((gt_ids ? (size_t)G : 0) + (pred_ids ? (size_t)S : 0));
    const size_t cells = ((size_t)G + 2) * ((size_t)S + 2);
    if (ids > kPqIdsMax || cells >= (1ull << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_pq_pairs: too many segments");
    if (table_bytes < cells * sizeof(int)) return mpf::fail(MPF_E_SHAPE, "seg_pq_pairs: table smaller than mpf_seg_pq_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const bool use_lds = ids + cells * sizeof(int) <= kPqLdsMax;
    const size_t lds = ids + (use_lds ? cells * sizeof(int) : 0);
    const int64_t nruns = (n + kPqRun - 1) / kPqRun;
    const int64_t want = (nruns + kPqT - 1) / kPqT;
    // LDS form: at most one workgroup per CU (every workgroup pays a zero and a flush pass over the histogram)
    const unsigned grid = (unsigned)std::min<int64_t>(want, use_lds ? mpf::cu_count() : 4 * mpf::cu_count());
    const bool rgb = gt_format == 1;
    mpf::prof_begin(st);
    mpf::set_kernel(use_lds ? "seg_pq_pairs_kernel<lds>" : "seg_pq_pairs_kernel<global>");
#define MPF_PQ_LAUNCH(L, R)                                                                                                         \
    hipLaunchKernelGGL((seg_pq_pairs_kernel<L, R>), dim3(grid), dim3(kPqT), lds, st, pred, gt, n, gt_ids, G, gt_base, pred_ids, S, \
                       pred_base, void_id, table)
    if (use_lds) {
        static mpf::LdsAttr attr[2];
        const void* fn = rgb ? (const void*)seg_pq_pairs_kernel<true, true> : (const void*)seg_pq_pairs_kernel<true, false>;
        if (int e = mpf::ensure_dynamic_lds(fn, kPqLdsMax, attr[rgb ? 1 : 0])) return e;
        if (rgb) MPF_PQ_LAUNCH(true, true);
        else MPF_PQ_LAUNCH(true, false);
    } else {
        if (rgb) MPF_PQ_LAUNCH(false, true);
        else MPF_PQ_LAUNCH(false, false);
    }
#undef MPF_PQ_LAUNCH
    mpf::prof_end(use_lds ? "seg_pq_pairs_kernel<lds>" : "seg_pq_pairs_kernel<global>", st, (rgb ? 7.0 : 8.0) * n);
    return mpf::check(hipGetLastError(), "mpf_seg_pq_pairs");
}

extern "C" int mpf_seg_pq_match(int* table, size_t table_bytes, int G, int S, int K, const int* gt_cat, const int* gt_flags,
                                const int* pred_cat, int implicit, int64_t* tp, int64_t* fp, int64_t* fn, double* iou, int64_t* err,
                                void* stream)
{
    if (!table || !tp || !fp || !fn || !iou || !err) return mpf::fail(MPF_E_NULL, "seg_pq_match: NULL buffer");
    if (G < 0 || S < 0 || K <= 0) return mpf::fail(MPF_E_SHAPE, "seg_pq_match: need G, S >= 0 segments and K > 0 classes");
    if (implicit != 0 && implicit != 1) return mpf::fail(MPF_E_SHAPE, "seg_pq_match: implicit is 0 or 1");
    if (implicit && (G != K || S != K || gt_cat || pred_cat || gt_flags))
        return mpf::fail(MPF_E_SHAPE, "seg_pq_match: the implicit form has G == S == K and no segment tables");
    if (!implicit && ((G > 0 && !gt_cat) || (S > 0 && !pred_cat))) return mpf::fail(MPF_E_NULL, "seg_pq_match: NULL category table");
    const size_t cells = ((size_t)G + 2) * ((size_t)S + 2);
    const size_t lds = pq_match_lds_bytes(G, S, K);
    if (lds > kPqIdsMax || cells >= (1ull << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_pq_match: too many segments or classes");
    if (table_bytes < cells * sizeof(int)) return mpf::fail(MPF_E_SHAPE, "seg_pq_match: table smaller than mpf_seg_pq_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_pq_match_kernel");
    hipLaunchKernelGGL(seg_pq_match_kernel, dim3(1), dim3(kPqMatchT), lds, st, table, G, S, K, gt_cat, gt_flags, pred_cat, implicit,
                       (unsigned long long*)tp, (unsigned long long*)fp, (unsigned long long*)fn, iou, (unsigned long long*)err);
    mpf::prof_end("seg_pq_match_kernel", st, 12.0 * cells);
    return mpf::check(hipGetLastError(), "mpf_seg_pq_match");
}
