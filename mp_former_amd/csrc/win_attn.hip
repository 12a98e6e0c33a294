// Shifted-window attention of the Swin backbone as bf16 MFMA tiles for MI355X (gfx950):
//   out = softmax(scale q k^T + table[index(i, j), head] + shift_mask(i, j)) v     per (image, window, head), head dim 32
// Reference semantics: WindowAttention.forward and the roll / window_partition / window_reverse / roll around it in
// SwinTransformerBlock.forward (mask2former/modeling/backbone/swin.py:131-171, :235-295), with the attention mask of
// BasicLayer.forward (:413-440).
//
// The regime is the opposite of attn.hip: many tiny problems (at most 144 tokens x 32 dims), so ONE workgroup holds a whole
// (window, head) in LDS and registers and the N x N matrix never reaches memory in either direction:
//   * input is the qkv Linear's output [B, Hp, Wp, 3 C] on the padded, un-rolled map; the cyclic shift and the window partition
//     are index arithmetic: the token at rolled position (r, c) lives at ((r + shift) mod Hp, (c + shift) mod Wp);
//   * the bias index and the shift mask are computed from the two tokens' in-window coordinates and rolled regions (a 32-bit
//     code per token in LDS), the table column of the head is staged in LDS;
//   * S^T = K Q^T with v_mfma_f32_16x16x32_bf16 as in attn.hip: queries on the lane axis, so the row maximum and sum are per-lane
//     values and two cross-lane steps; a lane keeps its query's whole row (<= 5 steps x 8 keys) in registers: no online softmax;
//     the key order of attn.hip (key_of_row) makes a lane's 8 probabilities of a 32-key step its B fragment of the P V product;
//   * tokens are padded to whole 32-key steps inside the kernel: padded rows are zero in LDS, padded keys score -inf
//     (probability exactly 0), padded queries are never stored;
//   * backward: a query-tile phase (lse, delta, dQ and the fp32 dS sums of the table gradient) and a key-tile phase (dK, dV) per
//     window, the second recomputing S with the keys on the lane axis.  Workgroups are persistent per head over a fixed slice of
//     the windows; a lane owns its (i, j) sums in registers across the slice, the workgroup folds them into one partial of the
//     table's shape in a fixed order, and a second kernel adds the partials in a fixed order.  No atomics: two runs give the
//     same bits.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "win_attn_host.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kHD = kWinHD, kPitch = kWinRowPitch;
constexpr float kNegInf = -INFINITY;

// row i of S^T tile t of a 32-token step is token 8 (i >> 2) + 4 t + (i & 3): the 8 values a lane holds after the two tiles are
// the consecutive tokens 8 g .. 8 g + 7 (attn.hip)
__device__ __forceinline__ int key_of_row(int t, int i) { return ((i >> 2) << 3) + 4 * t + (i & 3); }
__device__ __forceinline__ float xmax(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xsum(float v)
{
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ bf16x8 lds8(const __hip_bfloat16* p) { return *reinterpret_cast<const bf16x8*>(p); }

struct WinParams {
    const __hip_bfloat16* qkv;      // [B, Hp, Wp, 3 C]
    const float* table;             // [(2 ws - 1)^2, heads]
    const __hip_bfloat16* out;      // [B, Hp, Wp, C] (backward: the forward's result)
    const __hip_bfloat16* dout;     // [B, Hp, Wp, C]
    __hip_bfloat16* dst;            // forward: out; backward: dqkv [B, Hp, Wp, 3 C]
    float* part;                    // [parts, heads, (2 ws - 1)^2]
    int Hp, Wp, heads, ws, shift, N, wcols, windows, items, parts;
    float scale;
};

// LDS carve-up shared by the two kernels: the small arrays first, the operands behind them
struct Small {
    float* tb; int* pos; int* tok; float* lse; float* delta; __hip_bfloat16* ops;
    __device__ Small(char* base, int table_rows, int KP)
    {
        tb = (float*)base;
        pos = (int*)(base + (table_rows + 3) / 4 * 16);
        tok = pos + KP; lse = (float*)(tok + KP); delta = lse + KP;
        ops = (__hip_bfloat16*)(delta + KP);
    }
};

// Per token of the window of `item`: its position in the un-rolled map and its code = in-window (row (2 ws - 1) + col) | rolled
// region << 16.  Tokens N .. KP - 1 repeat the last one: their addresses and table indices stay in range, nothing of them is used.
__device__ __forceinline__ void fill_tokens(const WinParams& p, const Small& s, int item, int KP)
{
    const int b = item / p.windows, w = item - b * p.windows;
    const int wr = w / p.wcols, wc = w - wr * p.wcols;
    for (int i = threadIdx.x; i < KP; i += blockDim.x) {
        const int ii = min(i, p.N - 1), ti = ii / p.ws, tj = ii - ti * p.ws;
        const int r = wr * p.ws + ti, c = wc * p.ws + tj;
        int y = r + p.shift, x = c + p.shift;
        if (y >= p.Hp) y -= p.Hp;
        if (x >= p.Wp) x -= p.Wp;
        int region = 0;
        if (p.shift) region = 3 * (r < p.Hp - p.ws ? 0 : r < p.Hp - p.shift ? 1 : 2) + (c < p.Wp - p.ws ? 0 : c < p.Wp - p.shift ? 1 : 2);
        s.pos[i] = (b * p.Hp + y) * p.Wp + x;
        s.tok[i] = (ti * (2 * p.ws - 1) + tj) | (region << 16);
    }
}

// scale * acc + bias + mask of (query code tq, key code tk)
__device__ __forceinline__ float score(float acc, int tq, int tk, const float* tb, int off, float scale)
{
    const float bias = tb[(tq & 0xFFFF) - (tk & 0xFFFF) + off];
    return acc * scale + bias + ((tq >> 16) != (tk >> 16) ? -100.f : 0.f);
}

__device__ __forceinline__ void st4(__hip_bfloat16* dst, const f32x4& v, float mul)
{
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (__bf16)(v[r] * mul);
    *reinterpret_cast<bf16x4*>(dst) = o;
}

// One 16-byte piece per thread and trip of the 32 dims of a token row of `src` (token stride `stride`, head offset included):
// row-major copy into rows (pitch kPitch) and / or transposed copy into cols (pitch VP); rows N .. KP - 1 are zero
__device__ __forceinline__ void stage(const __hip_bfloat16* src, int stride, const int* pos, int N, int KP, int VP,
                                      __hip_bfloat16* rows, __hip_bfloat16* cols)
{
    for (int ch = threadIdx.x; ch < KP * 4; ch += blockDim.x) {
        const int row = ch >> 2, piece = ch & 3;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (int64_t)pos[row] * stride + 8 * piece);
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16x8 u = row < N ? v : z;
        if (rows) *reinterpret_cast<bf16x8*>(rows + row * kPitch + 8 * piece) = u;
        if (cols) {
#pragma unroll
            for (int e = 0; e < 8; ++e) *reinterpret_cast<__bf16*>(cols + (8 * piece + e) * VP + row) = u[e];
        }
    }
}

// The scores of query c16 of tile qt against every key: sc[st][j] = key 32 st + 8 g + j; -> (row maximum, sum of exp(s - max))
template <int STEPS>
__device__ __forceinline__ void score_row(float (&sc)[STEPS][8], const bf16x8 bq, const __hip_bfloat16* sK, const int* tok, const float* tb,
                                          int tq, int off, float scale, int N, int c16, int g, float& mx, float& l)
{
    mx = kNegInf;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bf16x8 ak = lds8(sK + (32 * st + key_of_row(t, c16)) * kPitch + 8 * g);
            const f32x4 z = {0, 0, 0, 0};
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, bq, z, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kj = 32 * st + 8 * g + 4 * t + r;
                const float s = score(acc[r], tq, tok[kj], tb, off, scale);
                sc[st][4 * t + r] = kj < N ? s : kNegInf;
                mx = fmaxf(mx, sc[st][4 * t + r]);
            }
        }
    }
    mx = xmax(mx);              // (key 0 is alive and in the query's own region or 100 below it: the maximum is finite)
    l = 0.f;
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) l += __expf(sc[st][j] - mx);
    l = xsum(l);
}

template <int STEPS>
__global__ __launch_bounds__(64 * kWinFwdWaves) void win_attn_fwd_kernel(WinParams p)
{
    extern __shared__ __attribute__((aligned(16))) char s_raw[];
    constexpr int KP = 32 * STEPS, VP = KP + 8;
    const int T = (2 * p.ws - 1) * (2 * p.ws - 1), off = (p.ws - 1) * 2 * p.ws, C = p.heads * kHD;
    const Small s(s_raw, T, KP);
    __hip_bfloat16* sK = s.ops;
    __hip_bfloat16* sVT = sK + KP * kPitch;
    const int lane = threadIdx.x & 63, c16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = blockIdx.y;
    fill_tokens(p, s, blockIdx.x, KP);
    for (int t = threadIdx.x; t < T; t += blockDim.x) s.tb[t] = p.table[t * p.heads + h];
    __syncthreads();
    stage(p.qkv + C + h * kHD, 3 * C, s.pos, p.N, KP, VP, sK, nullptr);
    stage(p.qkv + 2 * C + h * kHD, 3 * C, s.pos, p.N, KP, VP, nullptr, sVT);
    __syncthreads();
    const int tiles = (p.N + 15) / 16;
    for (int qt = wave; qt < tiles; qt += kWinFwdWaves) {
        const int qi = 16 * qt + c16, qc = min(qi, p.N - 1);
        const bf16x8 bq = *reinterpret_cast<const bf16x8*>(p.qkv + (int64_t)s.pos[qc] * 3 * C + h * kHD + 8 * g);
        float sc[STEPS][8], mx, l;
        score_row<STEPS>(sc, bq, sK, s.tok, s.tb, s.tok[qc], off, p.scale, p.N, c16, g, mx, l);
        f32x4 o[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
            bf16x8 bp;
#pragma unroll
            for (int j = 0; j < 8; ++j) bp[j] = (__bf16)__expf(sc[st][j] - mx);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sVT + (16 * dt + c16) * VP + 32 * st + 8 * g), bp, o[dt], 0, 0, 0);
        }
        // O^T C layout: lane (query c16, g) holds d = 16 dt + 4 g + r
        if (qi < p.N) {
            const float inv = 1.f / l;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) st4(p.dst + (int64_t)s.pos[qi] * C + h * kHD + 16 * dt + 4 * g, o[dt], inv);
        }
    }
}

// One wave per 16-token tile: blockDim.x = 64 * tiles
template <int STEPS>
__global__ __launch_bounds__(64 * 2 * STEPS) void win_attn_bwd_kernel(WinParams p)
{
    extern __shared__ __attribute__((aligned(16))) char s_raw[];
    constexpr int KP = 32 * STEPS, VP = KP + 8;
    const int T = (2 * p.ws - 1) * (2 * p.ws - 1), off = (p.ws - 1) * 2 * p.ws, C = p.heads * kHD;
    const Small s(s_raw, T, KP);
    __hip_bfloat16* sQ = s.ops;
    __hip_bfloat16* sK = sQ + KP * kPitch;
    __hip_bfloat16* sV = sK + KP * kPitch;
    __hip_bfloat16* sDO = sV + KP * kPitch;
    __hip_bfloat16* sQT = sDO + KP * kPitch;
    __hip_bfloat16* sKT = sQT + kHD * VP;
    __hip_bfloat16* sDOT = sKT + kHD * VP;
    const int lane = threadIdx.x & 63, c16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = blockIdx.y, N = p.N;
    const int ti = 16 * wave + c16;                     // this lane's token: a query in the first phase, a key in the second
    for (int t = threadIdx.x; t < T; t += blockDim.x) s.tb[t] = p.table[t * p.heads + h];
    for (int i = threadIdx.x; i < KP; i += blockDim.x) { s.lse[i] = 0.f; s.delta[i] = 0.f; }
    float tacc[STEPS][8];                               // sum over this workgroup's windows of dS[query ti][key 32 st + 8 g + j]
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) tacc[st][j] = 0.f;

    for (int item = blockIdx.x; item < p.items; item += p.parts) {
        __syncthreads();                                // the previous window's operands are no longer read
        fill_tokens(p, s, item, KP);
        __syncthreads();
        stage(p.qkv + h * kHD, 3 * C, s.pos, N, KP, VP, sQ, sQT);
        stage(p.qkv + C + h * kHD, 3 * C, s.pos, N, KP, VP, sK, sKT);
        stage(p.qkv + 2 * C + h * kHD, 3 * C, s.pos, N, KP, VP, sV, nullptr);
        stage(p.dout + h * kHD, C, s.pos, N, KP, VP, sDO, sDOT);
        __syncthreads();
        const int tc = min(ti, N - 1), code = s.tok[tc];
        const int64_t at = s.pos[tc];
        // ---- queries on the lane axis: lse, delta, dQ, the dS sums ------------------------------------------------------
        {
            const bf16x8 bq = lds8(sQ + ti * kPitch + 8 * g), bdo = lds8(sDO + ti * kPitch + 8 * g);
            const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(p.out + at * C + h * kHD + 8 * g);
            float delta = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) delta += (float)bdo[e] * (float)o8[e];
            delta = xsum(delta);                        // (a padded query has dO = 0 in LDS: delta = 0)
            float sc[STEPS][8], mx, l;
            score_row<STEPS>(sc, bq, sK, s.tok, s.tb, code, off, p.scale, N, c16, g, mx, l);
            const float lse = mx + __logf(l);
            if (g == 0) { s.lse[ti] = lse; s.delta[ti] = delta; }
            f32x4 dq[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (int st = 0; st < STEPS; ++st) {
                bf16x8 bds;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bf16x8 av = lds8(sV + (32 * st + key_of_row(t, c16)) * kPitch + 8 * g);
                    const f32x4 z = {0, 0, 0, 0};
                    const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bdo, z, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pr = __expf(sc[st][4 * t + r] - lse);          // a padded key: exp(-inf) = 0
                        const float ds = pr * (dp[r] - delta);
                        tacc[st][4 * t + r] += ti < N ? ds : 0.f;
                        bds[4 * t + r] = (__bf16)(ds * p.scale);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sKT + (16 * dt + c16) * VP + 32 * st + 8 * g), bds, dq[dt], 0, 0, 0);
            }
            if (ti < N) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) st4(p.dst + at * 3 * C + h * kHD + 16 * dt + 4 * g, dq[dt], 1.f);
            }
        }
        __syncthreads();                                // lse and delta of every query
        // ---- keys on the lane axis: dK, dV ------------------------------------------------------------------------------
        {
            const bf16x8 bk = lds8(sK + ti * kPitch + 8 * g), bv = lds8(sV + ti * kPitch + 8 * g);
            f32x4 dk[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, dv[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (int st = 0; st < STEPS; ++st) {
                bf16x8 bp, bds;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int row = (32 * st + key_of_row(t, c16)) * kPitch + 8 * g;
                    const f32x4 z = {0, 0, 0, 0};
                    const f32x4 sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sQ + row), bk, z, 0, 0, 0);
                    const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sDO + row), bv, z, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int qi = 32 * st + 8 * g + 4 * t + r;
                        const bool dead = qi >= N || ti >= N;
                        const float sv = score(sacc[r], s.tok[qi], code, s.tb, off, p.scale);
                        const float pr = dead ? 0.f : __expf(sv - s.lse[qi]);
                        const float ds = dead ? 0.f : pr * (dp[r] - s.delta[qi]);
                        bp[4 * t + r] = (__bf16)pr;
                        bds[4 * t + r] = (__bf16)(ds * p.scale);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const int col = (16 * dt + c16) * VP + 32 * st + 8 * g;
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sDOT + col), bp, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds8(sQT + col), bds, dk[dt], 0, 0, 0);
                }
            }
            if (ti < N) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    st4(p.dst + at * 3 * C + C + h * kHD + 16 * dt + 4 * g, dk[dt], 1.f);
                    st4(p.dst + at * 3 * C + 2 * C + h * kHD + 16 * dt + 4 * g, dv[dt], 1.f);
                }
            }
        }
    }
    // ---- the dS sums of the slice, folded into the table's shape in a fixed order ---------------------------------------
    __syncthreads();
    float* acc = (float*)s.ops;                         // [16 * waves, KP] over the operands, which are dead now
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ti * KP + 32 * st + 8 * g + j] = tacc[st][j];
    __syncthreads();
    const int side = 2 * p.ws - 1;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const int dr = t / side - (p.ws - 1), dc = t % side - (p.ws - 1);       // (query row - key row, query col - key col)
        float sum = 0.f;
        for (int ri = max(0, dr); ri < min(p.ws, p.ws + dr); ++ri)
            for (int ci = max(0, dc); ci < min(p.ws, p.ws + dc); ++ci) sum += acc[(ri * p.ws + ci) * KP + (ri - dr) * p.ws + (ci - dc)];
        p.part[((int64_t)blockIdx.x * p.heads + h) * T + t] = sum;
    }
}

// dtable[t, h] = the partials of (t, h) added in part order
__global__ __launch_bounds__(256) void win_attn_table_fold_kernel(const float* __restrict__ part, float* __restrict__ dtable, int parts, int heads,
                                                                   int T)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * heads) return;
    const int t = idx / heads, h = idx - t * heads;
    float sum = 0.f;
    for (int q = 0; q < parts; ++q) sum += part[((int64_t)q * heads + h) * T + t];
    dtable[idx] = sum;
}

}  // namespace

static WinParams win_params(const WinAttnProblem& pr, const void* qkv, const float* table, float scale)
{
    WinParams p = {};
    p.qkv = (const __hip_bfloat16*)qkv; p.table = table; p.scale = scale;
    p.Hp = pr.Hp; p.Wp = pr.Wp; p.heads = pr.heads; p.ws = pr.ws; p.shift = pr.shift; p.N = pr.N();
    p.wcols = pr.Wp / pr.ws; p.windows = pr.windows(); p.items = pr.items(); p.parts = pr.parts();
    return p;
}

// The launch of either direction: the kernel of the problem's step count with `lds` bytes of dynamic LDS
template <class Kernels>
static int win_launch(const char* name, const WinAttnProblem& pr, const WinParams& p, dim3 grid, dim3 block, size_t lds, double bytes,
                      double flops, hipStream_t st, Kernels&& kernels)
{
    int err = 0;
    mpf::with_int_of<1, 2, 3, 4, 5>(pr.steps(), [&](auto S) {
        static mpf::LdsAttr slots;
        auto kfn = kernels(S);
        if ((err = mpf::ensure_dynamic_lds((const void*)kfn, lds, slots))) return;
        mpf::prof_begin(st);
        mpf::set_kernel(name);
        hipLaunchKernelGGL(kfn, grid, block, lds, st, p);
        mpf::prof_end(name, st, bytes, flops);
    });
    return err;
}

extern "C" size_t mpf_win_attn_workspace_bytes(int B, int Hp, int Wp, int heads, int ws)
{
    const WinAttnProblem pr{B, Hp, Wp, heads, ws, 0};
    return pr.sizes_ok() && ws >= 2 && ws <= kWinMaxWs && Hp % ws == 0 && Wp % ws == 0 ? pr.workspace_bytes() : 0;
}

extern "C" int mpf_win_attn_forward(const void* qkv, const float* table, void* out, int B, int Hp, int Wp, int heads, int head_dim, int ws,
                                    int shift, float scale, void* stream)
{
    const WinAttnProblem pr{B, Hp, Wp, heads, ws, shift};
    if (int e = mpf::win_attn_check("win_attn_forward", pr, {qkv, table, out}, head_dim)) return e;
    WinParams p = win_params(pr, qkv, table, scale);
    p.dst = (__hip_bfloat16*)out;
    if (int e = win_launch("win_attn_fwd_kernel", pr, p, dim3(pr.items(), heads), dim3(64 * kWinFwdWaves), pr.fwd_lds(), pr.forward_bytes(),
                           pr.flops(2), (hipStream_t)stream, [](auto S) { return win_attn_fwd_kernel<decltype(S)::value>; }))
        return e;
    return mpf::check(hipGetLastError(), "mpf_win_attn_forward");
}

extern "C" int mpf_win_attn_backward(const void* qkv, const float* table, const void* out, const void* dout, void* dqkv, float* dtable, int B,
                                     int Hp, int Wp, int heads, int head_dim, int ws, int shift, float scale, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    const WinAttnProblem pr{B, Hp, Wp, heads, ws, shift};
    if (int e = mpf::win_attn_check("win_attn_backward", pr, {qkv, table, out, dout, dqkv, dtable, workspace}, head_dim)) return e;
    if (workspace_bytes < pr.workspace_bytes()) return mpf::failf(MPF_E_SHAPE, "win_attn_backward", "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    WinParams p = win_params(pr, qkv, table, scale);
    p.out = (const __hip_bfloat16*)out; p.dout = (const __hip_bfloat16*)dout; p.dst = (__hip_bfloat16*)dqkv; p.part = (float*)workspace;
    if (int e = win_launch("win_attn_bwd_kernel", pr, p, dim3(pr.parts(), heads), dim3(64 * pr.tiles()), pr.bwd_lds(), pr.backward_bytes(),
                           pr.flops(7), st, [](auto S) { return win_attn_bwd_kernel<decltype(S)::value>; }))
        return e;
    hipLaunchKernelGGL(win_attn_table_fold_kernel, dim3((pr.table_rows() * heads + 255) / 256), dim3(256), 0, st, (const float*)workspace, dtable,
                       pr.parts(), heads, pr.table_rows());
    return mpf::check(hipGetLastError(), "mpf_win_attn_backward");
}
