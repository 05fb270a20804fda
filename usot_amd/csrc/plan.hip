// Launch plans: the native per-frame runtime.
//
// A tracked frame is ~70 dependent kernel launches of a few microseconds each; issued one
// by one from Python the host, not the GPU, sets the frame rate.  A plan records the whole
// sequence once (descriptors with baked device pointers into the engine's static
// workspace), replays it from C++ with no per-launch Python, and can be captured into a
// hipGraph so that a frame costs one hipGraphLaunch.  Independent branches of the head
// (the cls / reg / memory chains, shortcut convs of the backbone) may be placed on side
// "lanes": extra streams forked from and joined to the main stream with events, which
// capture turns into parallel graph branches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <functional>
#include <new>
#include <utility>
#include <vector>
#include "usot_hip.h"
#include "common.h"

namespace {

// The numbers are frozen and documented beside usot_plan_op_info in include/usot_hip.h: drivers and scripts match on them.
enum Kind {
    K_CONV = 0, K_STEM = 1, K_POOL = 2, K_GDW = 3, K_CONF = 4, K_PRROI = 5, K_PERM = 6, K_DECODE = 7, K_FORK = 8, K_JOIN = 9,
    K_ROWS = 10, K_CONVB = 11, K_CVTB = 12, K_POOLB = 13, K_STEMB = 14, K_ROWSM = 15, K_THIN = 16, K_STEMP = 17, K_PWPAIR = 18,
    K_PW1 = 19, K_SC3 = 20, K_PW3 = 21, K_PANEL = 22, K_PANELP = 23, K_HALO = 24, K_KSTREAM = 25, K_CKSTREAM = 26, K_BNECK1 = 27,
    K_BNECKT = 28, K_CONVPW = 29, K_CONVPWP = 30, K_CONVPWO = 31, K_ROWSAG = 32, K_DECB = 33, K_ROWSAGB = 34, K_CROPB = 35
};

constexpr int kLanes = 4;     // lane 0 is the caller's stream

using Launch = std::function<int(hipStream_t)>;

// An op is a kind, a lane and a closure that owns a copy of every argument (descriptors and by-pointer arrays included) and calls
// the immediate entry point its adder chose; fork / join carry no closure.
struct Op {
    Kind kind;
    int lane;
    Launch launch;
    usot_conv_desc conv;          // K_CONV (first problem) / K_CONVB only: what usot_plan_op_info reports
};

struct Plan {
    std::vector<Op> ops;
    int cur_lane = 0;
    hipStream_t side[kLanes] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> events;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool captured = false;
};

int issue(Plan *pl, hipStream_t main_stream, bool lanes, hipEvent_t *marks = nullptr, int reps = 1)
{
    hipStream_t st[kLanes];
    st[0] = main_stream;
    for (int k = 1; k < kLanes; ++k) st[k] = lanes ? pl->side[k] : main_stream;
    size_t ev = 0;
    size_t opi = 0;
    for (const Op &op : pl->ops) {
        hipStream_t s = st[op.lane];
        int rc = USOT_OK;
        if (marks && hipEventRecord(marks[opi], s) != hipSuccess) return USOT_ELAUNCH;
        ++opi;
        for (int rep = 0; rep < reps && rc == USOT_OK; ++rep)
        switch (op.kind) {
        case K_FORK:      // lane op.lane waits for everything issued so far on lane 0
            if (lanes && op.lane != 0) {
                if (ev >= pl->events.size()) return USOT_ESTATE;
                hipEvent_t e = pl->events[ev++];
                if (hipEventRecord(e, st[0]) != hipSuccess) return USOT_ELAUNCH;
                if (hipStreamWaitEvent(st[op.lane], e, 0) != hipSuccess) return USOT_ELAUNCH;
            }
            break;
        case K_JOIN:      // lane 0 waits for lane op.lane
            if (lanes && op.lane != 0) {
                if (ev >= pl->events.size()) return USOT_ESTATE;
                hipEvent_t e = pl->events[ev++];
                if (hipEventRecord(e, st[op.lane]) != hipSuccess) return USOT_ELAUNCH;
                if (hipStreamWaitEvent(st[0], e, 0) != hipSuccess) return USOT_ELAUNCH;
            }
            break;
        default: rc = op.launch ? op.launch(s) : USOT_ESTATE; break;      // (only fork / join come without a closure)
        }
        if (rc != USOT_OK) return rc;
    }
    if (marks && hipEventRecord(marks[opi], main_stream) != hipSuccess) return USOT_ELAUNCH;
    return USOT_OK;
}

int prepare_lanes(Plan *pl)
{
    size_t need = 0;
    bool any = false;
    for (const Op &op : pl->ops) {
        if (op.kind == K_FORK || op.kind == K_JOIN) ++need;
        if (op.lane != 0) any = true;
    }
    if (!any) return USOT_OK;
    for (int k = 1; k < kLanes; ++k)
        if (!pl->side[k] && hipStreamCreateWithFlags(&pl->side[k], hipStreamNonBlocking) != hipSuccess)
            return USOT_ENOMEM;
    while (pl->events.size() < need) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return USOT_ENOMEM;
        pl->events.push_back(e);
    }
    return USOT_OK;
}

// Appends an op to an open plan.  `info`: the conv descriptor usot_plan_op_info reports (K_CONV, K_CONVB).
int push(void *plan, Kind k, Launch launch, const usot_conv_desc *info = nullptr)
{
    Plan *pl = (Plan *)plan;
    if (!pl || pl->captured) return USOT_ESTATE;
    pl->ops.push_back(Op{k, pl->cur_lane, std::move(launch), info ? *info : usot_conv_desc{}});
    return USOT_OK;
}

// The first n elements of a caller's array, by value (the rest zero): what a closure keeps of a by-pointer argument.
template <size_t N, class T>
std::array<T, N> take(const T *src, int n)
{
    std::array<T, N> a{};
    for (int i = 0; i < n; ++i) a[i] = src[i];
    return a;
}

// last_count NULL: the static launch
int add_groupdw(void *plan, const usot_groupdw_desc *d, int nseg, const int32_t *last_count)
{
    if (!d || nseg < 1 || nseg > 3) return USOT_EINVAL;
    const auto g = take<3>(d, nseg);
    return push(plan, K_GDW, [=](hipStream_t s) { return usot_groupdw_multi_dyn_f32(s, g.data(), nseg, last_count); });
}

// map NULL: no slot map
int add_conf_reduce(void *plan, const float *cv, float *out, int B, int M, int P, int C, const int32_t *map)
{
    return push(plan, K_CONF, [=](hipStream_t s) { return usot_conf_fusion_reduce_map_f32(s, cv, out, B, M, P, C, map); });
}

// mem_map NULL: every picked row is copied
int add_rows_append_gather(void *plan, const float *const *fresh, float *const *bank, float *const *picked, const int32_t *row_len,
                           const int32_t *idx_dev, int n_pick, int slot_pos, int32_t *mem_map)
{
    if (!fresh || !bank || !picked || !row_len || !idx_dev || n_pick < 1 || n_pick > 32 || slot_pos < 0) return USOT_EINVAL;
    const auto f = take<4>(fresh, 4);
    const auto b = take<4>(bank, 4);
    const auto p = take<3>(picked, 3);
    const auto len = take<4>(row_len, 4);
    if (mem_map)
        return push(plan, K_ROWSAG, [=](hipStream_t s) {
            return usot_rows_append_gather_dedupe_f32(s, f.data(), b.data(), p.data(), len.data(), idx_dev, n_pick, slot_pos, mem_map);
        });
    return push(plan, K_ROWSAG, [=](hipStream_t s) {
        return usot_rows_append_gather_f32(s, f.data(), b.data(), p.data(), len.data(), idx_dev, n_pick, slot_pos);
    });
}

}  // namespace

extern "C" void *usot_plan_create(void) { return new (std::nothrow) Plan(); }

extern "C" void usot_plan_destroy(void *plan)
{
    Plan *pl = (Plan *)plan;
    if (!pl) return;
    if (pl->exec) (void)hipGraphExecDestroy(pl->exec);
    if (pl->graph) (void)hipGraphDestroy(pl->graph);
    for (hipEvent_t e : pl->events) (void)hipEventDestroy(e);
    for (int k = 1; k < kLanes; ++k)
        if (pl->side[k]) (void)hipStreamDestroy(pl->side[k]);
    delete pl;
}

extern "C" int usot_plan_size(void *plan) { return plan ? (int)((Plan *)plan)->ops.size() : USOT_EINVAL; }

extern "C" int usot_plan_add_conv(void *plan, const usot_conv_desc *d)
{
    if (!d) return USOT_EINVAL;
    return usot_plan_add_conv_batch(plan, d, 1);
}

extern "C" int usot_plan_add_conv_batch(void *plan, const usot_conv_desc *d, int n)
{
    if (!d || n < 1 || n > 4) return USOT_EINVAL;
    if (n == 1) {
        const usot_conv_desc one = *d;
        return push(plan, K_CONV, [=](hipStream_t s) { return usot_conv2d_f32(s, &one); }, d);
    }
    const auto c = take<4>(d, n);
    return push(plan, K_CONV, [=](hipStream_t s) { return usot_conv2d_batch_f32(s, c.data(), n); }, d);
}

extern "C" int usot_plan_add_conv_lp(void *plan, const usot_conv_desc *d, int dtype, int out_f32)
{
    if (!d) return USOT_EINVAL;
    const usot_conv_desc c = *d;
    return push(plan, K_CONVB, [=](hipStream_t s) { return usot_conv2d_lp(s, &c, dtype, out_f32); }, d);
}

extern "C" int usot_plan_add_conv_bf16(void *plan, const usot_conv_desc *d) { return usot_plan_add_conv_lp(plan, d, 0, 0); }

extern "C" int usot_plan_add_pw_pair(void *plan, const usot_pw_pair_desc *d, int dtype)
{
    if (!d || !(dtype == 3 ? usot_pw_pair_f32s_supported(d->CM, d->CO, d->CN) : dtype == 2 ? usot_pw_pair_f32_supported(d->CM, d->CO, d->CN) : usot_pw_pair_supported(d->CM, d->CO, d->CN))) return USOT_EINVAL;
    // the fp32 (256, 1024, 256) pair exists in the channel-sliced form only: it needs M small enough to slice AND a workspace —
    // refuse it here, at build time, not at the first run / graph capture
    if ((dtype == 2 || dtype == 3) && d->CM == 256 && !(d->ws && usot_pw_pair_f32_ws_floats(d->M, d->CM, d->CO, d->CN) > 0)) return USOT_EINVAL;
    const usot_pw_pair_desc pw = *d;
    if (dtype == 3) return push(plan, K_PWPAIR, [=](hipStream_t s) { return usot_pw_pair_f32s(s, &pw); });
    if (dtype == 2) return push(plan, K_PWPAIR, [=](hipStream_t s) { return usot_pw_pair_f32(s, &pw); });
    return push(plan, K_PWPAIR, [=](hipStream_t s) { return usot_pw_pair_lp(s, &pw, dtype); });
}

extern "C" int usot_plan_add_pw_single(void *plan, const float *x, const float *wp, const float *b, const float *res, float *y,
                                       int M, int K, int N, int act)
{
    if (!usot_pw_single_f32_supported(K, N)) return USOT_EINVAL;
    return push(plan, K_PW1, [=](hipStream_t s) { return usot_pw_single_f32(s, x, wp, b, res, y, M, K, N, act); });
}

extern "C" int usot_plan_add_conv3x3_halo(void *plan, const void *x, const void *w, const float *bias, void *y,
                                          int N, int H, int W, int Cin, int Cout, int act, int dtype)
{
    if (!usot_conv3x3_halo_supported(Cin, Cout)) return USOT_EINVAL;
    return push(plan, K_HALO, [=](hipStream_t s) { return usot_conv3x3_halo_lp(s, x, w, bias, y, N, H, W, Cin, Cout, act, dtype); });
}

extern "C" int usot_plan_add_bneck_first(void *plan, const usot_bneck_desc *d, int dtype)
{
    if (!d || (dtype != 0 && dtype != 1)) return USOT_EINVAL;
    const usot_bneck_desc bn = *d;
    return push(plan, K_BNECK1, [=](hipStream_t s) { return usot_bneck_first_lp(s, &bn, dtype); });
}

extern "C" int usot_plan_add_bneck_tail(void *plan, const usot_bneck_desc *d, int Cnext, int dtype)
{
    if (!d || (dtype != 0 && dtype != 1) || !usot_bneck_tail_supported(64, 256, Cnext)) return USOT_EINVAL;
    const usot_bneck_desc bn = *d;
    return push(plan, K_BNECKT, [=](hipStream_t s) { return usot_bneck_tail_lp(s, &bn, Cnext, dtype); });
}

extern "C" int usot_plan_add_conv_kstream(void *plan, const void *x, const void *w, const float *bias, void *y,
                                          int N, int H, int W, int Cin, int Cout, int stride, int pad, int dil, int act, int dtype)
{
    if (!usot_conv_kstream_supported(Cin, Cout, 3, 3)) return USOT_EINVAL;
    return push(plan, K_CKSTREAM, [=](hipStream_t s) {
        return usot_conv_kstream_lp(s, x, w, bias, y, N, H, W, Cin, Cout, stride, pad, dil, act, dtype);
    });
}

extern "C" int usot_plan_add_pw_kstream(void *plan, const void *x, const void *w, const float *bias, void *y,
                                        long M, int K, int N, int act, int dtype)
{
    if (!usot_pw_kstream_supported(K, N)) return USOT_EINVAL;
    return push(plan, K_KSTREAM, [=](hipStream_t s) { return usot_pw_kstream_lp(s, x, w, bias, y, M, K, N, act, dtype); });
}

extern "C" int usot_plan_add_pw_panel_pair(void *plan, const usot_pw_pair_desc *d, int dtype)
{
    if (!d || !usot_pw_panel_pair_supported(d->CM, d->CO, d->CN) || (dtype != 0 && dtype != 1)) return USOT_EINVAL;
    const usot_pw_pair_desc pw = *d;
    return push(plan, K_PANELP, [=](hipStream_t s) { return usot_pw_panel_pair_lp(s, &pw, dtype); });
}

extern "C" int usot_plan_add_conv_pw(void *plan, const usot_conv_desc *c2, const void *w3, const float *b3, const void *res, void *y,
                                     int dtype)
{
    if (!c2 || !usot_conv_pw_supported(c2->Cin, c2->Cout, 4 * c2->Cout) || (dtype != 0 && dtype != 1)) return USOT_EINVAL;
    const usot_conv_desc c = *c2;
    return push(plan, K_CONVPW, [=](hipStream_t s) { return usot_conv_pw_lp(s, &c, w3, b3, res, y, dtype); });
}

extern "C" int usot_plan_add_conv_pw_pair(void *plan, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype)
{
    if (!c2 || !d || !usot_conv_pw_pair_supported(d->CM, d->CO, d->CN) || (dtype != 0 && dtype != 1)) return USOT_EINVAL;
    const usot_conv_desc c = *c2;
    const usot_pw_pair_desc pw = *d;
    return push(plan, K_CONVPWP, [=](hipStream_t s) { return usot_conv_pw_pair_lp(s, &c, &pw, dtype); });
}

extern "C" int usot_plan_add_conv_pw_ov(void *plan, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype, void *ws)
{
    if (!c2 || !d || !ws || !usot_conv_pw_ov_supported(d->CM, d->CO, d->CN) || (dtype != 0 && dtype != 1)) return USOT_EINVAL;
    const usot_conv_desc c = *c2;
    const usot_pw_pair_desc pw = *d;
    return push(plan, K_CONVPWO, [=](hipStream_t s) { return usot_conv_pw_ov_lp(s, &c, &pw, dtype, ws); });
}

extern "C" int usot_plan_add_pw_panel(void *plan, const void *x, const void *w, const float *bias, const void *res, void *y,
                                      int M, int K, int N, int act, int dtype)
{
    if (!usot_pw_panel_supported(K, N)) return USOT_EINVAL;
    return push(plan, K_PANEL, [=](hipStream_t s) { return usot_pw_panel_lp(s, x, w, bias, res, y, M, K, N, act, dtype); });
}

extern "C" int usot_plan_add_pw_triple(void *plan, const float *x, const float *w2p, const float *b2, const usot_pw_pair_desc *d,
                                       int Nb, int H, int W, int Cin, int OH, int OW, int pad_h, int pad_w, int dil_h, int dil_w)
{
    if (!d || !usot_pw_triple_f32_supported(Cin, d->CM, d->CO, d->CN)) return USOT_EINVAL;
    const usot_pw_pair_desc pw = *d;
    return push(plan, K_PW3, [=](hipStream_t s) {
        return usot_pw_triple_f32(s, x, w2p, b2, &pw, Nb, H, W, Cin, OH, OW, pad_h, pad_w, dil_h, dil_w);
    });
}

extern "C" int usot_plan_add_stream_conv3x3(void *plan, const float *x, const float *wp, const float *b, const float *res, float *y,
                                            int Nb, int H, int W, int Cin, int OH, int OW, int N, int pad_h, int pad_w, int dil_h,
                                            int dil_w, int act)
{
    if (!usot_stream_conv3x3_f32_supported(Cin, N)) return USOT_EINVAL;
    return push(plan, K_SC3, [=](hipStream_t s) {
        return usot_stream_conv3x3_f32(s, x, wp, b, res, y, Nb, H, W, Cin, OH, OW, N, pad_h, pad_w, dil_h, dil_w, act);
    });
}

extern "C" int usot_plan_add_cvt_lp(void *plan, const float *src, void *dst, int64_t n, int dtype)
{
    return push(plan, K_CVTB, [=](hipStream_t s) { return usot_cvt_f32_to_lp(s, src, dst, n, dtype); });
}

extern "C" int usot_plan_add_stem_pool(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                                       int N, int H, int W, int OH, int OW, int PH, int PW)
{
    return usot_plan_add_stem_pool_ind(plan, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, nullptr);
}

extern "C" int usot_plan_add_stem_pool_ind(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                                           int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev)
{
    return usot_plan_add_stem_pool_mu(plan, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, xptr_dev, 0.f, 0.f, 0.f);
}

extern "C" int usot_plan_add_stem_pool_mu(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                                          int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev,
                                          float mu0, float mu1, float mu2)
{
    return push(plan, K_STEMP, [=](hipStream_t s) {
        return usot_stem_pool_mu_f32(s, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, xptr_dev, mu0, mu1, mu2);
    });
}

extern "C" int usot_plan_add_thin_conv(void *plan, const usot_conv_desc *d, int n)
{
    if (!d || n < 1 || n > 4) return USOT_EINVAL;
    const auto c = take<4>(d, n);
    return push(plan, K_THIN, [=](hipStream_t s) { return usot_thin_conv3x3_f32(s, c.data(), n); });
}

extern "C" int usot_plan_add_rows_copy_multi(void *plan, int nseg, const float *const *src, const int32_t *idx_dev,
                                             float *const *dst, int n_rows, const int32_t *row_len, int scatter,
                                             int32_t *stash_next)
{
    if (nseg < 1 || nseg > 4 || !src || !dst || !row_len) return USOT_EINVAL;
    const auto from = take<4>(src, nseg);
    const auto to = take<4>(dst, nseg);
    const auto len = take<4>(row_len, nseg);
    return push(plan, K_ROWSM, [=](hipStream_t s) {
        return usot_rows_copy_multi_f32(s, nseg, from.data(), idx_dev, to.data(), n_rows, len.data(), scatter, stash_next);
    });
}

extern "C" int usot_plan_add_rows_append_gather(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                                const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos)
{
    return add_rows_append_gather(plan, fresh, bank, picked, row_len, idx_dev, n_pick, slot_pos, nullptr);
}

extern "C" int usot_plan_add_rows_append_gather_dedupe(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                                       const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos,
                                                       int32_t *mem_map)
{
    if (!mem_map || ((size_t)mem_map & 3)) return USOT_EINVAL;
    return add_rows_append_gather(plan, fresh, bank, picked, row_len, idx_dev, n_pick, slot_pos, mem_map);
}

// lock-step multi-video tracking (csrc/multitrack.hip): the plan adders check their arguments as the eager entry points do
extern "C" int usot_plan_add_decode_batch(void *plan, const float *cls, const float *cls_mem, const float *bbox, const double *window,
                                          double *out, int B, int S, int instance_size, int stride, float ratio, double penalty_k,
                                          double window_influence, const void *ctl, float *roi_out)
{
    if (!plan || !cls || !cls_mem || !bbox || !window || !out || !ctl || !roi_out || B < 1 || B > 65535 || S < 1 || S > 32)
        return USOT_EINVAL;
    return push(plan, K_DECB, [=](hipStream_t s) {
        return usot_decode_batch_f32(s, cls, cls_mem, bbox, window, out, B, S, instance_size, stride, ratio, penalty_k,
                                     window_influence, ctl, roi_out);
    });
}

extern "C" int usot_plan_add_rows_append_gather_batch(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                                      const int32_t *row_len, const void *ctl, int B, int n_pick, int bank_rows)
{
    if (!plan || !fresh || !bank || !picked || !row_len || !ctl || B < 1 || B > 65535 || n_pick < 1 || n_pick > 32 || bank_rows < 1)
        return USOT_EINVAL;
    for (int q = 0; q < 4; ++q) {
        if (!fresh[q] || !bank[q] || row_len[q] <= 0 || (row_len[q] & 3)) return USOT_EINVAL;
        if (q && !picked[q - 1]) return USOT_EINVAL;
    }
    const auto f = take<4>(fresh, 4);
    const auto b = take<4>(bank, 4);
    const auto p = take<3>(picked, 3);
    const auto len = take<4>(row_len, 4);
    return push(plan, K_ROWSAGB, [=](hipStream_t s) {
        return usot_rows_append_gather_batch_f32(s, f.data(), b.data(), p.data(), len.data(), ctl, B, n_pick, bank_rows);
    });
}

extern "C" int usot_plan_add_crop_resize_batch(void *plan, const void *ctl, float *out, int B, int S)
{
    if (!plan || !ctl || !out || B < 1 || B > 65535 || S < 1 || S > 4096) return USOT_EINVAL;
    return push(plan, K_CROPB, [=](hipStream_t s) { return usot_crop_resize_batch_u8_f32(s, ctl, out, B, S); });
}

extern "C" int usot_plan_add_stem_pool_lp(void *plan, const float *x, const void *wfrag, const float *bias, void *y,
                                          int N, int H, int W, int OH, int OW, int PH, int PW, int dtype,
                                          float mu0, float mu1, float mu2)
{
    return push(plan, K_STEMB, [=](hipStream_t s) {
        return usot_stem_pool_lp(s, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, dtype, mu0, mu1, mu2);
    });
}

extern "C" int usot_plan_add_cvt_bf16(void *plan, const float *src, void *dst, int64_t n) { return usot_plan_add_cvt_lp(plan, src, dst, n, 0); }

extern "C" int usot_plan_add_maxpool_lp(void *plan, const void *x, void *y, int N, int H, int W, int C, int OH, int OW, int dtype)
{
    return push(plan, K_POOLB, [=](hipStream_t s) { return usot_maxpool3x3s2_lp(s, x, y, N, H, W, C, OH, OW, dtype); });
}

extern "C" int usot_plan_add_maxpool_bf16(void *plan, const void *x, void *y, int N, int H, int W, int C, int OH, int OW)
{
    return usot_plan_add_maxpool_lp(plan, x, y, N, H, W, C, OH, OW, 0);
}

extern "C" int usot_plan_add_groupdw(void *plan, const usot_groupdw_desc *d)
{
    if (!d) return USOT_EINVAL;
    return usot_plan_add_groupdw_multi(plan, d, 1);
}

extern "C" int usot_plan_add_groupdw_multi(void *plan, const usot_groupdw_desc *d, int nseg)
{
    return add_groupdw(plan, d, nseg, nullptr);
}

extern "C" int usot_plan_add_groupdw_multi_dyn(void *plan, const usot_groupdw_desc *d, int nseg, const int32_t *last_count)
{
    return add_groupdw(plan, d, nseg, last_count);
}

extern "C" int usot_plan_add_groupdw_multi_lp(void *plan, const usot_groupdw_desc *d, int nseg, int out_dtype)
{
    if (!d || nseg < 1 || nseg > 3 || (out_dtype != 1 && out_dtype != 2)) return USOT_EINVAL;
    const auto g = take<3>(d, nseg);
    return push(plan, K_GDW, [=](hipStream_t s) { return usot_groupdw_multi_lp(s, g.data(), nseg, out_dtype); });
}

extern "C" int usot_plan_add_conf_reduce_lp(void *plan, const void *cv, int in_dtype, void *out, int B, int M, int P, int C, int out_dtype)
{
    if ((out_dtype != 1 && out_dtype != 2) || in_dtype < 0 || in_dtype > 2) return USOT_EINVAL;
    return push(plan, K_CONF, [=](hipStream_t s) { return usot_conf_fusion_reduce_lp(s, cv, in_dtype, out, B, M, P, C, out_dtype); });
}

extern "C" int usot_plan_add_stem(void *plan, const float *x, const float *w, const float *bias, float *y,
                                  int N, int H, int W, int OH, int OW)
{
    return usot_plan_add_stem_mu(plan, x, w, bias, y, N, H, W, OH, OW, 0.f, 0.f, 0.f);
}

extern "C" int usot_plan_add_stem_mu(void *plan, const float *x, const float *w, const float *bias, float *y,
                                     int N, int H, int W, int OH, int OW, float mu0, float mu1, float mu2)
{
    return push(plan, K_STEM, [=](hipStream_t s) { return usot_stem_conv_mu_f32(s, x, w, bias, y, N, H, W, OH, OW, mu0, mu1, mu2); });
}

extern "C" int usot_plan_add_maxpool(void *plan, const float *x, float *y, int N, int H, int W, int C,
                                     int OH, int OW)
{
    return push(plan, K_POOL, [=](hipStream_t s) { return usot_maxpool3x3s2_f32(s, x, y, N, H, W, C, OH, OW); });
}

extern "C" int usot_plan_add_conf_reduce(void *plan, const float *cv, float *out, int B, int M, int P, int C)
{
    return add_conf_reduce(plan, cv, out, B, M, P, C, nullptr);
}

extern "C" int usot_plan_add_conf_reduce_map(void *plan, const float *cv, float *out, int B, int M, int P, int C, const int32_t *map)
{
    return add_conf_reduce(plan, cv, out, B, M, P, C, map);
}

extern "C" int usot_plan_add_prroi(void *plan, const float *feat, const float *rois, float *out,
                                   int R, int C, int H, int W, int PH, int PW, float scale,
                                   int64_t f_sb, int64_t f_sc, int64_t f_sh, int64_t f_sw,
                                   int64_t o_sr, int64_t o_sc, int64_t o_sh, int64_t o_sw)
{
    return push(plan, K_PRROI, [=](hipStream_t s) {
        return usot_prroi_pool_forward_f32(s, feat, rois, out, R, C, H, W, PH, PW, scale, f_sb, f_sc, f_sh, f_sw, o_sr, o_sc, o_sh, o_sw);
    });
}

extern "C" int usot_plan_add_permute(void *plan, const float *src, float *dst, int D0, int D1, int D2, int D3,
                                     int64_t s0, int64_t s1, int64_t s2, int64_t s3)
{
    return push(plan, K_PERM, [=](hipStream_t s) { return usot_permute4_f32(s, src, dst, D0, D1, D2, D3, s0, s1, s2, s3); });
}

/* tsz_dev: device double[2] = target size * scale_z, refreshed by the host per frame;
 * roi_out: optional device float[5], receives (0, pool_label_search(best box)).          */
extern "C" int usot_plan_add_decode(void *plan, const float *cls, const float *cls_mem, const float *bbox,
                                    const double *window, double *out, int S, int instance_size, int stride,
                                    float ratio, double penalty_k, double window_influence,
                                    const double *tsz_dev, float *roi_out)
{
    return push(plan, K_DECODE, [=](hipStream_t s) {
        return usot_decode_dev_f32(s, cls, cls_mem, bbox, window, out, S, instance_size, stride, ratio, penalty_k, window_influence,
                                   tsz_dev, roi_out);
    });
}

extern "C" int usot_plan_add_rows_copy(void *plan, const float *src, const int32_t *idx_dev, float *dst,
                                       int n_rows, int row_len, int scatter)
{
    return push(plan, K_ROWS, [=](hipStream_t s) { return usot_rows_copy_f32(s, src, idx_dev, dst, n_rows, row_len, scatter); });
}

extern "C" int usot_plan_fork(void *plan, int lane)
{
    Plan *pl = (Plan *)plan;
    if (!pl || lane < 0 || lane >= kLanes) return USOT_EINVAL;
    pl->cur_lane = lane;
    return push(plan, K_FORK, nullptr);
}

extern "C" int usot_plan_join(void *plan, int lane)
{
    Plan *pl = (Plan *)plan;
    if (!pl || lane < 0 || lane >= kLanes) return USOT_EINVAL;
    pl->cur_lane = lane;
    const int rc = push(plan, K_JOIN, nullptr);
    if (rc == USOT_OK) pl->cur_lane = 0;
    return rc;
}

extern "C" int usot_plan_capture(void *plan, void *stream)
{
    Plan *pl = (Plan *)plan;
    if (!pl || pl->captured || pl->ops.empty()) return USOT_ESTATE;
    int rc = prepare_lanes(pl);
    if (rc != USOT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return USOT_ELAUNCH;
    rc = issue(pl, s, true);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != USOT_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc != USOT_OK ? rc : USOT_ELAUNCH;
    }
    if (hipGraphInstantiate(&pl->exec, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(g);
        return USOT_ELAUNCH;
    }
    pl->graph = g;
    pl->captured = true;
    return USOT_OK;
}

extern "C" int usot_plan_run(void *plan, void *stream)
{
    Plan *pl = (Plan *)plan;
    if (!pl) return USOT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (pl->captured) return hipGraphLaunch(pl->exec, s) == hipSuccess ? USOT_OK : USOT_ELAUNCH;
    return issue(pl, s, false);
}

/* Per-op timing with HIP events on the launching stream: issues the plan `frames` times in
 * program order on `stream` (lanes ignored, no graph) with an event before every op, each op
 * launched `reps` times back to back (amortises the event's own cost), and returns the mean
 * milliseconds per launch in ms_per_op[usot_plan_size()].
 * Blocks until done.  Used by bench.py for the roofline object.                           */
extern "C" int usot_plan_profile(void *plan, void *stream, int frames, int reps, float *ms_per_op)
{
    Plan *pl = (Plan *)plan;
    if (!pl || !ms_per_op || frames < 1 || reps < 1 || pl->ops.empty()) return USOT_EINVAL;
    const size_t n = pl->ops.size();
    std::vector<hipEvent_t> marks(n + 1);
    for (auto &e : marks)
        if (hipEventCreate(&e) != hipSuccess) return USOT_ENOMEM;
    std::vector<double> acc(n, 0.0);
    hipStream_t s = (hipStream_t)stream;
    int rc = USOT_OK;
    for (int f = 0; f < frames && rc == USOT_OK; ++f) {
        rc = issue(pl, s, false, marks.data(), reps);
        if (rc != USOT_OK) break;
        if (hipStreamSynchronize(s) != hipSuccess) { rc = USOT_ELAUNCH; break; }
        for (size_t i = 0; i < n; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, marks[i], marks[i + 1]) != hipSuccess) { rc = USOT_ELAUNCH; break; }
            acc[i] += ms;
        }
    }
    for (auto &e : marks) (void)hipEventDestroy(e);
    if (rc == USOT_OK)
        for (size_t i = 0; i < n; ++i) ms_per_op[i] = (float)(acc[i] / frames / reps);
    return rc;
}

/* info[0..3] = kind (the table in include/usot_hip.h), tile, ksplit, groups of op i; for fp32 convs the tile is the one the
 * launcher would pick now. */
extern "C" int usot_plan_op_info(void *plan, int i, int *info)
{
    Plan *pl = (Plan *)plan;
    if (!pl || !info || i < 0 || i >= (int)pl->ops.size()) return USOT_EINVAL;
    const Op &op = pl->ops[i];
    info[0] = (int)op.kind; info[1] = 0; info[2] = 1; info[3] = 1;
    if (op.kind == K_CONVB) { info[1] = op.conv.tile; }
    if (op.kind == K_CONV) {
        info[1] = usot_conv_resolve_tile(&op.conv);
        info[2] = op.conv.ksplit > 1 ? op.conv.ksplit : 1;
        info[3] = op.conv.groups;
    }
    return USOT_OK;
}
