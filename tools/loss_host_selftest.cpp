// Stand-alone run of csrc/loss_host.h on the host, for a sanitizer build: the record's arithmetic, the route functions and
// loss_check over every single and every pairwise variation of a good problem per entry, with the values of the fault table of
// tools/record_loss_host.py (zeros, negatives, 65 536 rows, w = 16 385, 38 401 points, 65 536 frames, INT_MAX, planes around the
// LDS limits).  It launches nothing and needs no device.  Build and run from the repository root:
//   hipcc -x hip -std=c++17 --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I mp_former_amd/csrc tools/loss_host_selftest.cpp -o /tmp/loss_host_selftest && /tmp/loss_host_selftest
// It asserts what must hold for every problem the check lets through: an LDS route never asks for more than the 160 KiB of a
// workgroup, the bands of the dense backward cover the plane within their limit, the grids are non-empty and within grid.y.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "loss_host.h"

namespace mpf {
static char t_err[256];
int fail(int code, const char* msg) { snprintf(t_err, sizeof(t_err), "%s", msg); return code; }
int failf(int code, const char* who, const char* what) { snprintf(t_err, sizeof(t_err), "%s: %s", who, what); return code; }
}  // namespace mpf

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (last text: %s)\n", __FILE__, __LINE__, #c, mpf::t_err); abort(); } } while (0)

namespace {
constexpr int kIntMax = 0x7fffffff;
constexpr size_t kWorkgroupLds = 160 * 1024;
const void* const kPtr = (const void*)0x7f0000001000;

struct Field { int LossProblem::*m; std::vector<int> values; };
const std::vector<Field> kFields = {
    {&LossProblem::dtype, {MPF_F32, MPF_F64, MPF_BF16, MPF_U8, MPF_BITS, 99}},
    {&LossProblem::h, {-1, 0, 5, 256, 264, 280, 400, kIntMax}},
    {&LossProblem::w, {-1, 0, 7, 176, 256, 16384, 16385, 32769, kIntMax}},
    {&LossProblem::n, {-1, 0, 3, 9, 65535, 65536, kIntMax}},
    {&LossProblem::P, {-1, 0, 12800, 12801, 38400, 38401, kIntMax}},
    {&LossProblem::H, {-1, 0, 5, kIntMax}},
    {&LossProblem::W, {-1, 0, 7, kIntMax}},
    {&LossProblem::gt_dtype, {MPF_BF16, MPF_U8, MPF_BITS, 99}},
    {&LossProblem::grad_dtype, {MPF_F32, MPF_BF16, 99}},
    {&LossProblem::chunks, {-1, 0, 256, 257, kIntMax}},
    {&LossProblem::M, {-1, 0, 16384, 16385, 37888, 37889, 40960, 40961, kIntMax}},
    {&LossProblem::k, {-1, 0, 701, kIntMax}},
    {&LossProblem::P_out, {-1, 0, 99, kIntMax}},
    {&LossProblem::F, {-1, 0, 1, 65535, 65536, kIntMax}},
    {&LossProblem::Tmax, {-1, 0, 100000, kIntMax}},
    {&LossProblem::G, {-1, 0, 1, 2, 3, 4, 5, kIntMax}},
};

long g_ok = 0, g_rejected = 0, g_lds = 0;

LossProblem good(LossEntry e)
{
    LossProblem p(e, MPF_BF16, 16, 24, 12, 100);
    p.H = 8; p.W = 20; p.chunks = 8; p.M = 700; p.k = 100; p.P_out = 103; p.Tmax = 5; p.G = 6;
    if (e == LossEntry::cost_clip) { p.F = 3; p.stride_f = 384; }
    return p;
}

void exercise(const char* who, const LossProblem& p)
{
    const size_t need = p.workspace_bytes();
    REQUIRE(loss_check(who, p, {kPtr, nullptr}) == MPF_E_NULL);
    const int e = loss_check(who, p, {kPtr, kPtr}, {kPtr}, kPtr, need);
    if (need) REQUIRE(loss_check(who, p, {kPtr}, {}, kPtr, need - 1) < 0 && loss_check(who, p, {kPtr}, {}, nullptr, need) < 0);
    if (e) { REQUIRE(e < 0 && mpf::t_err[0]); ++g_rejected; return; }
    ++g_ok;
    if (p.empty()) return;
    REQUIRE(p.bytes() >= 0.0 && p.bytes(LossRoute::lds) >= 0.0 && p.xs_bytes() > 0);
    const dim3 grids[] = {p.sample_grid(), p.fwd_grid(), p.bwd_grid(), p.cost_grid(), p.fold_grid()};
    for (const dim3& g : grids) REQUIRE(g.x > 0 && g.y > 0);
    switch (p.entry) {
    case LossEntry::point_sample: case LossEntry::backward: REQUIRE(p.sample_grid().y <= (unsigned)kGridY && p.bwd_grid().y <= (unsigned)kGridY); break;
    case LossEntry::forward:
        if (mask_loss_fwd_route(p) == LossRoute::lds) { ++g_lds; REQUIRE(p.fwd_lds() <= kWorkgroupLds && 4 * p.chunks <= kMcThreads); }
        break;
    case LossEntry::backward_dense:
        REQUIRE(p.max_rows() >= 2 && p.nb() >= 1 && (int64_t)p.nb() * p.band_rows() >= p.h && p.band_rows() <= p.max_rows());
        REQUIRE(p.band_lds() <= (size_t)kPlaneLds && p.band_grid().y <= (unsigned)kGridY);
        break;
    case LossEntry::sample_select: {
        const int pt = sample_select_pt(p.M);
        REQUIRE((pt == 16 || pt == 37 || pt == 40) && (int64_t)pt * kMcThreads >= p.M && p.select_lds(pt) <= kWorkgroupLds);
        break;
    }
    case LossEntry::cost: case LossEntry::cost_clip:
        REQUIRE(p.xs_bytes() <= kXsLds && p.cost_grid().y <= (unsigned)kGridY);
        if (match_cost_route(p) == LossRoute::lds) {
            ++g_lds;
            REQUIRE(p.cost_lds() <= kWorkgroupLds && p.P <= kCostPT * kCostThreads && p.cost_lds_grid().x > 0);
            REQUIRE((int64_t)p.cost_lds_grid().x * kCostRows >= p.n);              // every row has a workgroup
        }
        break;
    case LossEntry::select: break;
    }
}

void sweep(const char* who, LossEntry e)
{
    exercise(who, good(e));
    for (size_t a = 0; a < kFields.size(); ++a)
        for (int va : kFields[a].values) {
            LossProblem p = good(e);
            p.*kFields[a].m = va;
            if (e != LossEntry::cost_clip) p.F = 0;
            exercise(who, p);
            for (size_t b = a + 1; b < kFields.size(); ++b)
                for (int vb : kFields[b].values) {
                    LossProblem q = p;
                    q.*kFields[b].m = vb;
                    if (e != LossEntry::cost_clip) q.F = 0;          // only the clip entry sets F
                    exercise(who, q);
                    if (e == LossEntry::cost_clip) {
                        for (int64_t s : {(int64_t)-1, (int64_t)0, (int64_t)q.h * q.w - 1, (int64_t)q.h * q.w}) { q.stride_f = s; exercise(who, q); }
                    }
                }
        }
}
}  // namespace

int main()
{
    sweep("mpf_point_sample", LossEntry::point_sample);
    sweep("mpf_mask_loss_forward", LossEntry::forward);
    sweep("mpf_mask_loss_backward", LossEntry::backward);
    sweep("mpf_mask_loss_backward_dense", LossEntry::backward_dense);
    sweep("mpf_select_uncertain", LossEntry::select);
    sweep("mpf_sample_select_uncertain", LossEntry::sample_select);
    sweep("mpf_match_cost", LossEntry::cost);
    sweep("mpf_match_cost_clip", LossEntry::cost_clip);
    for (int n : {-1, 0, 1, 12, 600})
        for (int F : {-1, 0, 1, 3, 65535})
            for (int T : {-1, 0, 1, 5, 100}) {
                LossProblem p(LossEntry::cost_clip, MPF_BF16, 1, 1, n);
                p.F = F; p.Tmax = T;
                REQUIRE(p.workspace_bytes() == (n > 0 && F > 0 && T > 0 ? (size_t)n * F * (2 + 3 * T) * 4 : 0));
            }
    printf("loss_host.h: %ld problems accepted (%ld on an LDS route), %ld rejected\n", g_ok, g_lds, g_rejected);
    return 0;
}
