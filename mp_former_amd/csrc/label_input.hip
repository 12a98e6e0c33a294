// Training input on MI355X from LABEL MAPS: what the reference's panoptic and semantic mappers do on the CPU per image — resize the
// label map with nearest neighbour, count the labels of up to ten candidate crop windows (np.unique), pad, and build one dense mask
// per segment or class in a Python loop — from the decoded map, two index tables per image and a list of wanted ids.  Every result
// is an integer; nothing here has a floating-point value.
//
//   label_resample_kernel   one launch for a batch: out[b, y, x] = the id at source (ytab[y], xtab[x]) inside the valid extent, the
//                           pad id everywhere else on the canvas.  The tables (host-made, of the CROP WINDOW only) carry the nearest
//                           rule, so the kernel is a gather; flip_in mirrors the source column (large-scale jitter flips first),
//                           flip_out mirrors the valid columns of the result (the semantic mapper flips last).  Sources: uint8 or
//                           int32 label maps, or the RGB panoptic PNG read as R + 256 G + 65536 B.  One writer per element.
//   label_counts_kernel     per (image, candidate window, band of kBandRows window rows): the histogram of the labels in the band,
//                           read from the SOURCE through full-axis tables (the resized map is never formed), in LDS with integer
//                           atomics, then added to the zeroed [B, tries, K + 1] output with integer atomics: independent of order.
//                           The ignore label is skipped, labels outside 0 .. K-1 go to slot K.
//   label_bits_kernel       one image's id map and T <= kMaxIds wanted ids -> packed bits [T, nwords] (position p = x H + y, 64 per
//                           word) and areas [T].  A workgroup owns kTileWords consecutive words = a run of positions = a few
//                           columns; it reads those columns BY ROWS (lanes along x: the coalesced direction of the map), looks
//                           each id up in the sorted id list (binary search in LDS) and stores the list index as one byte at the
//                           position's place in LDS.  Then a wave owns a word: its 64 lanes read 64 consecutive bytes, and for each
//                           distinct index among them (ballot) one lane writes the word of that id's row(s).  The map is read once
//                           whatever T is; every non-zero word has one writer and zero words come from the cleared output; areas
//                           are popcounts folded in LDS and added with integer atomics.
//
// LDS: counts (kMaxClasses + 1) * 4 = 4100 B; bits kTileWords * 64 index bytes padded by 4 B per 256 (a column of a 1024-row map
// is 1024 B: unpadded, the byte stores of a wave that walks along a row would all land in one bank) + the id list = 6.4 KiB.
// Every table entry and window is checked on the host copy before a launch, so no index read on the device leaves a source image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mpf_common.h"

namespace {

constexpr int kT = 256;                    // threads per workgroup
constexpr int kMaxClasses = 1024;          // K of the counts: ADE20K-full has 847
constexpr int kBandRows = 32;              // window rows per workgroup of the counts
constexpr int kMaxTries = 16;
constexpr int kMaxIds = 255;               // wanted ids per launch of the bits: the list index is one byte, 255 = not wanted
constexpr int kTileWords = 64;             // words per workgroup of the bits: 4096 positions (1024 x 1024: one workgroup per CU)
constexpr int kLoads = 8;                  // map elements a thread has in flight
constexpr int kTilePos = kTileWords * 64;
constexpr int kTileLds = kTilePos + (kTilePos >> 8) * 4;

typedef MpfLabelRecord Rec;

struct BitsIds {                           // by value: the sorted wanted ids and the output row of each (duplicates are neighbours)
    int32_t id[kMaxIds + 1];
    uint8_t row[kMaxIds + 1];
};

__device__ __forceinline__ int read_label(const Rec& r, int sy, int sx)
{
    const unsigned char* row = (const unsigned char*)r.src + (int64_t)sy * r.src_stride;
    if (r.kind == MPF_LABEL_U8) return (int)row[sx];
    if (r.kind == MPF_LABEL_I32) return ((const int32_t*)row)[sx];
    const unsigned char* p = row + 3 * sx;
    return (int)p[0] + 256 * (int)p[1] + 65536 * (int)p[2];
}

__global__ __launch_bounds__(kT) void label_resample_kernel(const Rec* __restrict__ recs, const int* __restrict__ tab, int32_t* __restrict__ out,
                                                            int Hc, int Wc, int pad_id)
{
    const Rec r = recs[blockIdx.y];
    const int64_t plane = (int64_t)Hc * Wc;
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= plane) return;
    const int oy = (int)(i / Wc), ox = (int)(i - (int64_t)oy * Wc);
    int v = pad_id;
    if (oy < r.valid_h && ox < r.valid_w) {
        const int sy = tab[r.yt_off + oy];
        int sx = tab[r.xt_off + (r.flip_out ? r.valid_w - 1 - ox : ox)];
        if (r.flip_in) sx = r.src_w - 1 - sx;
        v = read_label(r, sy, sx);
    }
    out[(int64_t)blockIdx.y * plane + i] = v;
}

__global__ __launch_bounds__(kT) void label_counts_kernel(const Rec* __restrict__ recs, const int* __restrict__ tab, const int* __restrict__ win,
                                                          int32_t* __restrict__ counts, int tries, int K, int ignore_label)
{
    __shared__ int hist[kMaxClasses + 1];
    const int b = blockIdx.z, t = blockIdx.y;
    const int* w = win + ((int64_t)b * tries + t) * 4;
    const int y0 = w[0], x0 = w[1], ch = w[2], cw = w[3];
    const int r0 = blockIdx.x * kBandRows;
    if (r0 >= ch) return;                                    // (the whole workgroup: the grid is sized for the tallest window)
    const Rec r = recs[b];
    for (int i = threadIdx.x; i <= K; i += kT) hist[i] = 0;
    __syncthreads();
    const int rows = min(kBandRows, ch - r0);
    for (int i = threadIdx.x; i < rows * cw; i += kT) {
        const int yl = i / cw, xl = i - yl * cw;
        const int sy = tab[r.yt_off + y0 + r0 + yl];
        int sx = tab[r.xt_off + x0 + xl];
        if (r.flip_in) sx = r.src_w - 1 - sx;
        const int v = read_label(r, sy, sx);
        if (v == ignore_label) continue;
        atomicAdd(&hist[(unsigned)v < (unsigned)K ? v : K], 1);
    }
    __syncthreads();
    int32_t* o = counts + ((int64_t)b * tries + t) * (K + 1);
    for (int i = threadIdx.x; i <= K; i += kT)
        if (hist[i]) atomicAdd(&o[i], hist[i]);
}

__device__ __forceinline__ int lds_at(int q) { return q + ((q >> 8) << 2); }

__global__ __launch_bounds__(kT) void label_bits_kernel(const int32_t* __restrict__ map, int64_t stride, int H, int W, BitsIds ids, int T,
                                                        int64_t nwords, unsigned long long* __restrict__ bits, int32_t* __restrict__ areas)
{
    __shared__ unsigned char slot[kTileLds];
    __shared__ int sid[kMaxIds + 1];
    __shared__ int sarea[kMaxIds + 1];
    __shared__ unsigned char srow[kMaxIds + 1];
    const int64_t total = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * kTilePos;
    const int64_t p1 = p0 + kTilePos < total ? p0 + kTilePos : total;
    for (int i = threadIdx.x; i <= kMaxIds; i += kT) {
        sid[i] = ids.id[i];
        srow[i] = ids.row[i];
        sarea[i] = 0;
    }
    __syncthreads();
    // the columns x_lo .. x_hi hold the positions p0 .. p1 - 1; read them by rows and keep the positions inside the run
    const int x_lo = (int)(p0 / H), x_hi = (int)((p1 - 1) / H), ncol = x_hi - x_lo + 1;
    int y_lo = 0, y_hi = H;
    if (ncol == 1) {                                         // (a map taller than the tile: only the rows of the run)
        y_lo = (int)(p0 - (int64_t)x_lo * H);
        y_hi = (int)(p1 - (int64_t)x_lo * H);
    }
    const int n = (y_hi - y_lo) * ncol;                      // <= kTilePos + 2 H, and H < kTilePos where ncol > 1
    for (int base = 0; base < n; base += kT * kLoads) {
        // kLoads independent loads per thread first, then the searches: one load per iteration would serialise on its latency.
        // An index past n is clamped to n - 1 (a position of these columns and rows: in bounds) and its result dropped.
        int v[kLoads], q[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int i = base + u * kT + (int)threadIdx.x;
            const int ic = i < n ? i : n - 1;
            const int yl = ic / ncol, xl = ic - yl * ncol;
            const int y = y_lo + yl, x = x_lo + xl;
            const int64_t p = (int64_t)x * H + y;
            q[u] = (i < n && p >= p0 && p < p1) ? (int)(p - p0) : -1;
            v[u] = map[(int64_t)y * stride + x];
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            if (q[u] < 0) continue;
            int lo = 0, hi = T;                              // lower bound in the sorted list
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sid[mid] < v[u]) lo = mid + 1;
                else hi = mid;
            }
            slot[lds_at(q[u])] = (unsigned char)((lo < T && sid[lo] == v[u]) ? lo : kMaxIds);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int nw = (int)((p1 - p0 + 63) >> 6);
    for (int wi = threadIdx.x >> 6; wi < nw; wi += kT / 64) {
        const int q = wi * 64 + lane;
        const int s = p0 + q < p1 ? (int)slot[lds_at(q)] : kMaxIds;
        unsigned long long rest = __ballot(s != kMaxIds);
        while (rest) {                                       // one round per distinct wanted id among the 64 positions
            const int leader = __ffsll((long long)rest) - 1;
            const int cur = __shfl(s, leader);
            const unsigned long long m = __ballot(s == cur);
            rest &= ~m;
            if (lane == 0) {
                atomicAdd(&sarea[cur], __popcll(m));
                const int v = sid[cur];
                for (int j = cur; j < T && sid[j] == v; ++j)  // equal ids are neighbours in the list: equal rows
                    bits[(int64_t)srow[j] * nwords + (p0 >> 6) + wi] = m;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += kT) {
        int a = sarea[i];
        if (i > 0 && sid[i - 1] == sid[i]) {                 // a duplicate: the area was folded at the first of its run
            int j = i - 1;
            while (j > 0 && sid[j - 1] == sid[i]) --j;
            a = sarea[j];
        }
        if (a) atomicAdd(&areas[srow[i]], a);
    }
}

int bad(const char* who, const char* what) { return mpf::failf(MPF_E_SHAPE, who, what); }

int elem_bytes(int kind) { return kind == MPF_LABEL_U8 ? 1 : (kind == MPF_LABEL_I32 ? 4 : 3); }

// the source of a record, and one table of n entries indexing an axis of `in` entries
int check_source(const Rec& r, const char* who)
{
    if (!r.src) return mpf::failf(MPF_E_NULL, who, "NULL source map");
    if (r.kind != MPF_LABEL_U8 && r.kind != MPF_LABEL_I32 && r.kind != MPF_LABEL_RGB) return mpf::failf(MPF_E_DTYPE, who, "kind must be uint8, int32 or RGB");
    if (r.src_h <= 0 || r.src_w <= 0 || r.out_h <= 0 || r.out_w <= 0) return bad(who, "sizes must be positive");
    if (r.src_stride < (int64_t)elem_bytes(r.kind) * r.src_w) return bad(who, "row stride below one row of the source");
    if (r.kind == MPF_LABEL_I32 && (r.src_stride & 3)) return bad(who, "row stride of an int32 map must be a multiple of 4");
    if ((int64_t)r.src_stride * r.src_h >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "source map of 2^31 bytes or more");
    if (r.flip_in < 0 || r.flip_in > 1 || r.flip_out < 0 || r.flip_out > 1) return bad(who, "flip_in and flip_out must be 0 or 1");
    return 0;
}

int check_table(const int* tab, int64_t tab_len, int off, int n, int in, const char* who)
{
    if (off < 0 || (int64_t)off + n > tab_len) return bad(who, "an index table lies outside the table buffer");
    for (int i = 0; i < n; ++i)
        if (tab[off + i] < 0 || tab[off + i] >= in) return bad(who, "a table entry leaves the source map");
    return 0;
}

}  // namespace

extern "C" int mpf_label_counts_max_classes(void) { return kMaxClasses; }
extern "C" int mpf_label_counts_max_tries(void) { return kMaxTries; }
extern "C" int mpf_label_bits_max_ids(void) { return kMaxIds; }

extern "C" int mpf_label_resample(const MpfLabelRecord* recs_host, const MpfLabelRecord* recs_dev, const int32_t* tab_host,
                                  const int32_t* tab_dev, int64_t tab_len, int B, int32_t* out, int Hc, int Wc, int pad_id, void* stream)
{
    const char* who = "label_resample";
    if (B < 0 || Hc <= 0 || Wc <= 0 || tab_len < 0) return bad(who, "need B >= 0, a canvas Hc, Wc > 0 and tab_len >= 0");
    if (B == 0) return 0;
    if (!recs_host || !recs_dev || !tab_host || !tab_dev || !out) return mpf::fail(MPF_E_NULL, "label_resample: NULL buffer");
    if (B > 65535) return mpf::failf(MPF_E_TOO_LARGE, who, "B <= 65535 images");
    if ((int64_t)Hc * Wc >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "canvas of 2^31 elements or more");
    for (int b = 0; b < B; ++b) {
        const Rec& r = recs_host[b];
        if (int e = check_source(r, who)) return e;
        if (r.crop_h <= 0 || r.crop_w <= 0 || r.crop_h > Hc || r.crop_w > Wc) return bad(who, "canvas smaller than the crop");
        if (r.off_y < 0 || r.off_x < 0 || r.valid_h < 1 || r.valid_w < 1 || r.valid_h > r.crop_h || r.valid_w > r.crop_w ||
            r.off_y + r.valid_h > r.out_h || r.off_x + r.valid_w > r.out_w)
            return bad(who, "the valid extent must lie inside the crop and the resized map");
        if (int e = check_table(tab_host, tab_len, r.xt_off, r.valid_w, r.src_w, who)) return e;
        if (int e = check_table(tab_host, tab_len, r.yt_off, r.valid_h, r.src_h, who)) return e;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t plane = (int64_t)Hc * Wc;
    const dim3 grid((unsigned)((plane + kT - 1) / kT), (unsigned)B);
    mpf::prof_begin(st);
    mpf::set_kernel("label_resample_kernel");
    hipLaunchKernelGGL(label_resample_kernel, grid, dim3(kT), 0, st, recs_dev, (const int*)tab_dev, out, Hc, Wc, pad_id);
    mpf::prof_end("label_resample_kernel", st, (double)B * plane * 4.0);
    return mpf::check(hipGetLastError(), "mpf_label_resample");
}

extern "C" int mpf_label_window_counts(const MpfLabelRecord* recs_host, const MpfLabelRecord* recs_dev, const int32_t* tab_host,
                                       const int32_t* tab_dev, int64_t tab_len, const int32_t* win_host, const int32_t* win_dev, int B,
                                       int tries, int K, int ignore_label, int32_t* counts, void* stream)
{
    const char* who = "label_window_counts";
    if (B < 0 || tab_len < 0) return bad(who, "need B >= 0 and tab_len >= 0");
    if (tries < 1 || tries > kMaxTries) return bad(who, "tries outside 1 .. 16");
    if (K < 1 || K > kMaxClasses) return bad(who, "K outside 1 .. 1024 classes");
    if (B == 0) return 0;
    if (!recs_host || !recs_dev || !tab_host || !tab_dev || !win_host || !win_dev || !counts) return mpf::fail(MPF_E_NULL, "label_window_counts: NULL buffer");
    if (B > 65535) return mpf::failf(MPF_E_TOO_LARGE, who, "B <= 65535 images");
    int max_h = 1;
    for (int b = 0; b < B; ++b) {
        const Rec& r = recs_host[b];
        if (int e = check_source(r, who)) return e;
        if (int e = check_table(tab_host, tab_len, r.xt_off, r.out_w, r.src_w, who)) return e;
        if (int e = check_table(tab_host, tab_len, r.yt_off, r.out_h, r.src_h, who)) return e;
        for (int t = 0; t < tries; ++t) {
            const int32_t* w = win_host + ((int64_t)b * tries + t) * 4;
            if (w[0] < 0 || w[1] < 0 || w[2] < 1 || w[3] < 1 || (int64_t)w[0] + w[2] > r.out_h || (int64_t)w[1] + w[3] > r.out_w)
                return bad(who, "a window must lie inside the resized map");
            if ((int64_t)kBandRows * w[3] >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "window too wide");
            if (w[2] > max_h) max_h = w[2];
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((max_h + kBandRows - 1) / kBandRows), (unsigned)tries, (unsigned)B);
    mpf::prof_begin(st);
    mpf::set_kernel("label_counts_kernel");
    if (int e = mpf::check(hipMemsetAsync(counts, 0, (size_t)B * tries * (K + 1) * sizeof(int32_t), st), "mpf_label_window_counts")) return e;
    hipLaunchKernelGGL(label_counts_kernel, grid, dim3(kT), 0, st, recs_dev, (const int*)tab_dev, (const int*)win_dev, counts, tries, K, ignore_label);
    mpf::prof_end("label_counts_kernel", st, (double)B * tries * (K + 1) * 4.0);
    return mpf::check(hipGetLastError(), "mpf_label_window_counts");
}

extern "C" int mpf_label_bits(const int32_t* map, int64_t row_stride, int H, int W, const int32_t* ids_host, int T, int64_t* bits,
                              int32_t* areas, void* stream)
{
    const char* who = "label_bits";
    if (H <= 0 || W <= 0 || T < 0) return bad(who, "need H, W > 0 and T >= 0");
    if (row_stride < W) return bad(who, "row stride below W");
    if ((int64_t)H * W >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "H * W < 2^31");
    if (T > kMaxIds) return mpf::failf(MPF_E_TOO_LARGE, who, "T <= 255 ids per launch (the caller splits a longer list)");
    if (T == 0) return 0;
    if (!map || !ids_host || !bits || !areas) return mpf::fail(MPF_E_NULL, "label_bits: NULL buffer");
    BitsIds ids;
    int order[kMaxIds + 1];
    for (int i = 0; i < T; ++i) order[i] = i;
    std::stable_sort(order, order + T, [&](int a, int b) { return ids_host[a] < ids_host[b]; });
    for (int i = 0; i <= kMaxIds; ++i) {
        ids.id[i] = i < T ? ids_host[order[i]] : INT32_MAX;
        ids.row[i] = (uint8_t)(i < T ? order[i] : 0);
    }
    const int64_t nwords = ((int64_t)H * W + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("label_bits_kernel");
    // zero words come from the cleared output: the kernel writes the non-zero words only, each by one lane
    if (int e = mpf::check(hipMemsetAsync(bits, 0, (size_t)T * nwords * sizeof(int64_t), st), "mpf_label_bits")) return e;
    if (int e = mpf::check(hipMemsetAsync(areas, 0, (size_t)T * sizeof(int32_t), st), "mpf_label_bits")) return e;
    const dim3 grid((unsigned)((nwords + kTileWords - 1) / kTileWords));
    hipLaunchKernelGGL(label_bits_kernel, grid, dim3(kT), 0, st, map, row_stride, H, W, ids, T, nwords, (unsigned long long*)bits, areas);
    mpf::prof_end("label_bits_kernel", st, (double)H * W * 4.0 + (double)T * nwords * 8.0);
    return mpf::check(hipGetLastError(), "mpf_label_bits");
}
