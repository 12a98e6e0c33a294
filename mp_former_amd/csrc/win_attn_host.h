// Host-side record of the shifted-window attention family ("Shifted-window attention").  win_attn.hip holds the kernels,
// one launcher per direction and the three entry points: each fills one WinAttnProblem, the only place where the family's sizes,
// grids and LDS budgets are written, and checks once before any HIP call.
#pragma once
#include "mpf_common.h"

constexpr int kWinHD = 32;          // head dim
constexpr int kWinMaxWs = 12;       // window side: N = ws^2 <= 144 tokens
constexpr int kWinRowPitch = 40;    // bf16 per token row in LDS (32 + 8: 16-byte aligned rows, 20 banks apart)
constexpr int kWinFwdWaves = 4;     // waves per workgroup of the forward

struct WinAttnProblem {
    int B, Hp, Wp, heads, ws, shift;
    int N() const { return ws * ws; }                              // tokens of a window
    int tiles() const { return (N() + 15) / 16; }                  // 16-token tiles: query tiles of a wave, waves of the backward
    int steps() const { return (N() + 31) / 32; }                  // 32-key steps
    int KP() const { return 32 * steps(); }                        // tokens padded to whole steps (dead keys: probability exactly 0)
    int VP() const { return KP() + 8; }                            // bf16 per row of a transposed operand in LDS
    int C() const { return heads * kWinHD; }
    int windows() const { return (Hp / ws) * (Wp / ws); }
    int items() const { return B * windows(); }                    // (image, window)
    int table_rows() const { return (2 * ws - 1) * (2 * ws - 1); }
    // backward: `parts` persistent workgroups per head, each over the items part, part + parts, ...
    int parts() const { const int want = 512 / heads > 0 ? 512 / heads : 1; return items() < want ? items() : want; }
    size_t workspace_bytes() const { return mpf::align256((size_t)parts() * heads * table_rows() * sizeof(float)); }
    // LDS: the table column of the head, token positions, token codes, (lse, delta) | operands
    size_t small_bytes() const { return ((size_t)table_rows() + 3) / 4 * 16 + (size_t)KP() * 4 * sizeof(int); }
    size_t fwd_lds() const { return small_bytes() + ((size_t)KP() * kWinRowPitch + (size_t)kWinHD * VP()) * 2; }
    size_t bwd_operand_bytes() const { return ((size_t)4 * KP() * kWinRowPitch + (size_t)3 * kWinHD * VP()) * 2; }
    size_t bwd_acc_bytes() const { return (size_t)tiles() * 16 * KP() * sizeof(float); }     // the dS sums, over the dead operands
    size_t bwd_lds() const { return small_bytes() + (bwd_operand_bytes() > bwd_acc_bytes() ? bwd_operand_bytes() : bwd_acc_bytes()); }
    bool sizes_ok() const { return B > 0 && Hp > 0 && Wp > 0 && heads > 0; }
    // profiler records: qkv once and out once | qkv, out, dout once and dqkv once
    double forward_bytes() const { return 2.0 * B * Hp * Wp * C() * 4; }
    double backward_bytes() const { return 2.0 * B * Hp * Wp * C() * 8; }
    double flops(int products) const { return 2.0 * products * items() * heads * (double)N() * N() * kWinHD; }
};

namespace mpf {
// The check of the forward and backward entries
inline int win_attn_check(const char* who, const WinAttnProblem& p, std::initializer_list<const void*> required, int head_dim)
{
    if (any_null(required)) return failf(MPF_E_NULL, who, "NULL buffer");
    if (p.ws < 2 || p.ws > kWinMaxWs) return failf(MPF_E_SHAPE, who, "window size must be 2 .. 12");
    if (head_dim != kWinHD) return failf(MPF_E_SHAPE, who, "head_dim must be 32");
    if (p.shift < 0 || p.shift >= p.ws) return failf(MPF_E_SHAPE, who, "shift must be 0 .. ws - 1");
    if (!p.sizes_ok()) return failf(MPF_E_SHAPE, who, "bad sizes");
    if (p.Hp % p.ws || p.Wp % p.ws) return failf(MPF_E_SHAPE, who, "Hp and Wp must be multiples of the window size");
    if ((int64_t)p.B * p.Hp * p.Wp * 3 * p.C() >= ((int64_t)1 << 31)) return failf(MPF_E_TOO_LARGE, who, "qkv exceeds 2^31 elements");
    for (const void* b : required)
        if ((uintptr_t)b & 15) return failf(MPF_E_SHAPE, who, "buffers must be 16-byte aligned");
    return 0;
}
}  // namespace mpf
