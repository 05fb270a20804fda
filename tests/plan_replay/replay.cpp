// Replay check of the launch-plan runtime (usot_amd/csrc/plan.hip) that needs no GPU.
//
// The plan adders and an eager usot_plan_run make no HIP call, so plan.hip links against the recording stubs below instead of the
// kernels' launchers.  main() calls every usot_plan_add_* once accepted - with all-distinct integers, floats and doubles and a
// distinct offset into one fake arena for every pointer, so that a swapped argument shows - and once per rejection it has, frees
// every descriptor and array it handed over, and replays the plan.  Each stub prints its name and every argument (pointers as
// arena offsets, descriptors and arrays dereferenced, field by field): the output is deterministic, and
// tests/golden/plan_replay.txt holds it (tests/test_plan_replay.py).  A closure that kept the caller's pointer instead of a copy
// reads a scribbled, freed block: a changed line here, a use-after-free report under -fsanitize=address.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "usot_hip.h"

// ------------------------------------------------------------------ printing
static unsigned char arena[1 << 15];

static void put(const void *p)
{
    const ptrdiff_t o = (const unsigned char *)p - arena;
    if (!p) printf(" null");
    else if (o >= 0 && o < (ptrdiff_t)sizeof(arena)) printf(" @%td", o);
    else printf(" @outside");
}
static void put(int v) { printf(" %d", v); }
static void put(long v) { printf(" %ldL", v); }
static void put(float v) { printf(" %.9gf", v); }
static void put(double v) { printf(" %.17gd", v); }
static void put(const char *s) { printf(" %s", s); }

static void put(const usot_conv_desc &d);
static void put(const usot_pw_pair_desc &d);
static void put(const usot_bneck_desc &d);
static void put(const usot_groupdw_desc &d);
// a descriptor pointer is always printed dereferenced
template <class D> static void put(const D *d)
{
    if (d) put(*d);
    else printf(" null");
}
static void put(const float *p) { put((const void *)p); }
static void put(float *p) { put((const void *)p); }
static void put(const double *p) { put((const void *)p); }
static void put(double *p) { put((const void *)p); }
static void put(const int32_t *p) { put((const void *)p); }
static void put(int32_t *p) { put((const void *)p); }
static void put(void *p) { put((const void *)p); }

template <class T> struct Arr { const T *p; int n; };
template <class T> static Arr<T> arr(const T *p, int n) { return Arr<T>{p, n}; }
template <class T> static void put(Arr<T> a)
{
    printf(" [");
    for (int i = 0; i < a.n; ++i) put(a.p[i]);
    printf(" ]");
}
template <class... A> static void puts_(A... a) { (put(a), ...); }
template <class... A> static void line(const char *name, A... a)
{
    printf("%s", name);
    (put(a), ...);
    printf("\n");
}

static void put(const usot_conv_desc &d)
{
    printf(" conv{");
    puts_(d.x, d.w, d.bias, d.res, d.y, d.ws, d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad_h, d.pad_w,
          d.dil_h, d.dil_w, d.y_cstride, d.y_coff, d.res_cstride, d.res_coff, d.y_nchw, d.act, d.act2, d.act_split, d.groups,
          d.x_gs, d.w_gs, d.b_gs, d.y_gs, d.r_gs, d.ksplit, d.tile, d.w_frag, d.defer, d.w_scale, d.x_split, d.y_split, d.ovf,
          d.n_dyn, d.n_first);
    printf(" }");
}
static void put(const usot_pw_pair_desc &d)
{
    printf(" pair{");
    puts_(d.t2, d.w3p, d.res, d.w1, d.b3, d.b1, d.y, d.t, d.M, d.CM, d.CO, d.CN, d.act2, d.ws, d.t2_parts, d.res_parts, d.t2_bias,
          d.res_bias, d.ovf);
    printf(" }");
}
static void put(const usot_bneck_desc &d)
{
    printf(" bneck{");
    puts_(d.x, d.w1, d.w2, d.w3c, d.wn, d.b1, d.b2, d.b3c, d.bn, d.y, d.t, d.N, d.H, d.W);
    printf(" }");
}
static void put(const usot_groupdw_desc &d)
{
    printf(" gdw{");
    puts_(arr(d.x, 3), arr(d.z, 3), d.out, arr(d.hk, 3), arr(d.wk, 3), arr(d.x_cs, 3), arr(d.x_co, 3), arr(d.z_cs, 3),
          arr(d.z_co, 3), arr(d.wsm, 3), d.S, d.x_rep, d.OH, d.OW, d.C, d.cols_per_thread);
    printf(" }");
}
// ------------------------------------------------------------------ what main() scripts
static int g_supported = 1;      // answer of every *_supported query
static long g_ws_floats = 7;     // answer of usot_pw_pair_f32_ws_floats
static int g_tile = 42;          // answer of usot_conv_resolve_tile
static int g_calls = 0;          // launches since main() last cleared it
static int g_fail_at = 0;        // the launch (1-based) that answers USOT_ELAUNCH; 0 = none

static int done(void)
{
    ++g_calls;
    return g_calls == g_fail_at ? USOT_ELAUNCH : USOT_OK;
}

// ------------------------------------------------------------------ the 57 symbols plan.o leaves undefined
extern "C" {

#define QUERY(name, ...) { line(#name, __VA_ARGS__); return g_supported; }
int usot_pw_pair_supported(int CM, int CO, int CN) QUERY(usot_pw_pair_supported, CM, CO, CN)
int usot_pw_pair_f32_supported(int CM, int CO, int CN) QUERY(usot_pw_pair_f32_supported, CM, CO, CN)
int usot_pw_pair_f32s_supported(int CM, int CO, int CN) QUERY(usot_pw_pair_f32s_supported, CM, CO, CN)
int usot_pw_single_f32_supported(int K, int N) QUERY(usot_pw_single_f32_supported, K, N)
int usot_conv3x3_halo_supported(int Cin, int Cout) QUERY(usot_conv3x3_halo_supported, Cin, Cout)
int usot_bneck_tail_supported(int Cmid, int Cout, int Cnext) QUERY(usot_bneck_tail_supported, Cmid, Cout, Cnext)
int usot_conv_kstream_supported(int Cin, int Cout, int KH, int KW) QUERY(usot_conv_kstream_supported, Cin, Cout, KH, KW)
int usot_pw_kstream_supported(int K, int N) QUERY(usot_pw_kstream_supported, K, N)
int usot_pw_panel_supported(int K, int N) QUERY(usot_pw_panel_supported, K, N)
int usot_pw_panel_pair_supported(int CM, int CO, int CN) QUERY(usot_pw_panel_pair_supported, CM, CO, CN)
int usot_conv_pw_supported(int Cin, int CM, int CO) QUERY(usot_conv_pw_supported, Cin, CM, CO)
int usot_conv_pw_pair_supported(int CM, int CO, int CN) QUERY(usot_conv_pw_pair_supported, CM, CO, CN)
int usot_conv_pw_ov_supported(int CM, int CO, int CN) QUERY(usot_conv_pw_ov_supported, CM, CO, CN)
int usot_pw_triple_f32_supported(int Cin, int CM, int CO, int CN) QUERY(usot_pw_triple_f32_supported, Cin, CM, CO, CN)
int usot_stream_conv3x3_f32_supported(int Cin, int N) QUERY(usot_stream_conv3x3_f32_supported, Cin, N)
#undef QUERY

int64_t usot_pw_pair_f32_ws_floats(int M, int CM, int CO, int CN)
{
    line("usot_pw_pair_f32_ws_floats", M, CM, CO, CN);
    return g_ws_floats;
}

int usot_conv_resolve_tile(const usot_conv_desc *d)
{
    line("usot_conv_resolve_tile", d);
    return g_tile;
}

#define LAUNCH(name, ...) { line(#name, stream, __VA_ARGS__); return done(); }
int usot_conv2d_f32(void *stream, const usot_conv_desc *d) LAUNCH(usot_conv2d_f32, d)
int usot_conv2d_batch_f32(void *stream, const usot_conv_desc *d, int n) LAUNCH(usot_conv2d_batch_f32, arr(d, n), n)
int usot_thin_conv3x3_f32(void *stream, const usot_conv_desc *d, int n) LAUNCH(usot_thin_conv3x3_f32, arr(d, n), n)
int usot_conv2d_lp(void *stream, const usot_conv_desc *d, int dtype, int out_f32) LAUNCH(usot_conv2d_lp, d, dtype, out_f32)
int usot_cvt_f32_to_lp(void *stream, const float *src, void *dst, int64_t n, int dtype) LAUNCH(usot_cvt_f32_to_lp, src, dst, n, dtype)
int usot_maxpool3x3s2_lp(void *stream, const void *x, void *y, int N, int H, int W, int C, int OH, int OW, int dtype)
    LAUNCH(usot_maxpool3x3s2_lp, x, y, N, H, W, C, OH, OW, dtype)
int usot_stem_pool_lp(void *stream, const float *x, const void *wfrag, const float *bias, void *y, int N, int H, int W, int OH, int OW,
                      int PH, int PW, int dtype, float mu0, float mu1, float mu2)
    LAUNCH(usot_stem_pool_lp, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, dtype, mu0, mu1, mu2)
int usot_pw_pair_lp(void *stream, const usot_pw_pair_desc *d, int dtype) LAUNCH(usot_pw_pair_lp, d, dtype)
int usot_pw_pair_f32(void *stream, const usot_pw_pair_desc *d) LAUNCH(usot_pw_pair_f32, d)
int usot_pw_pair_f32s(void *stream, const usot_pw_pair_desc *d) LAUNCH(usot_pw_pair_f32s, d)
int usot_pw_panel_lp(void *stream, const void *x, const void *w, const float *bias, const void *res, void *y, int M, int K, int N,
                     int act, int dtype)
    LAUNCH(usot_pw_panel_lp, x, w, bias, res, y, M, K, N, act, dtype)
int usot_pw_panel_pair_lp(void *stream, const usot_pw_pair_desc *d, int dtype) LAUNCH(usot_pw_panel_pair_lp, d, dtype)
int usot_conv_pw_lp(void *stream, const usot_conv_desc *c2, const void *w3, const float *b3, const void *res, void *y, int dtype)
    LAUNCH(usot_conv_pw_lp, c2, w3, b3, res, y, dtype)
int usot_conv_pw_pair_lp(void *stream, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype)
    LAUNCH(usot_conv_pw_pair_lp, c2, d, dtype)
int usot_conv_pw_ov_lp(void *stream, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype, void *ws)
    LAUNCH(usot_conv_pw_ov_lp, c2, d, dtype, ws)
int usot_conv3x3_halo_lp(void *stream, const void *x, const void *w, const float *bias, void *y, int N, int H, int W, int Cin,
                         int Cout, int act, int dtype)
    LAUNCH(usot_conv3x3_halo_lp, x, w, bias, y, N, H, W, Cin, Cout, act, dtype)
int usot_bneck_first_lp(void *stream, const usot_bneck_desc *d, int dtype) LAUNCH(usot_bneck_first_lp, d, dtype)
int usot_bneck_tail_lp(void *stream, const usot_bneck_desc *d, int Cnext, int dtype) LAUNCH(usot_bneck_tail_lp, d, Cnext, dtype)
int usot_pw_kstream_lp(void *stream, const void *x, const void *w, const float *bias, void *y, long M, int K, int N, int act, int dtype)
    LAUNCH(usot_pw_kstream_lp, x, w, bias, y, M, K, N, act, dtype)
int usot_conv_kstream_lp(void *stream, const void *x, const void *w, const float *bias, void *y, int N, int H, int W, int Cin,
                         int Cout, int stride, int pad, int dil, int act, int dtype)
    LAUNCH(usot_conv_kstream_lp, x, w, bias, y, N, H, W, Cin, Cout, stride, pad, dil, act, dtype)
int usot_pw_single_f32(void *stream, const float *x, const float *wp, const float *b, const float *res, float *y, int M, int K,
                       int N, int act)
    LAUNCH(usot_pw_single_f32, x, wp, b, res, y, M, K, N, act)
int usot_pw_triple_f32(void *stream, const float *x, const float *w2p, const float *b2, const usot_pw_pair_desc *d, int Nb, int H,
                       int W, int Cin, int OH, int OW, int pad_h, int pad_w, int dil_h, int dil_w)
    LAUNCH(usot_pw_triple_f32, x, w2p, b2, d, Nb, H, W, Cin, OH, OW, pad_h, pad_w, dil_h, dil_w)
int usot_stream_conv3x3_f32(void *stream, const float *x, const float *wp, const float *b, const float *res, float *y, int Nb, int H,
                            int W, int Cin, int OH, int OW, int N, int pad_h, int pad_w, int dil_h, int dil_w, int act)
    LAUNCH(usot_stream_conv3x3_f32, x, wp, b, res, y, Nb, H, W, Cin, OH, OW, N, pad_h, pad_w, dil_h, dil_w, act)
int usot_stem_conv_mu_f32(void *stream, const float *x, const float *w, const float *bias, float *y, int N, int H, int W, int OH,
                          int OW, float mu0, float mu1, float mu2)
    LAUNCH(usot_stem_conv_mu_f32, x, w, bias, y, N, H, W, OH, OW, mu0, mu1, mu2)
int usot_stem_pool_mu_f32(void *stream, const float *x, const float *wfrag, const float *bias, float *y, int N, int H, int W, int OH,
                          int OW, int PH, int PW, const int32_t *xptr_dev, float mu0, float mu1, float mu2)
    LAUNCH(usot_stem_pool_mu_f32, x, wfrag, bias, y, N, H, W, OH, OW, PH, PW, xptr_dev, mu0, mu1, mu2)
int usot_maxpool3x3s2_f32(void *stream, const float *x, float *y, int N, int H, int W, int C, int OH, int OW)
    LAUNCH(usot_maxpool3x3s2_f32, x, y, N, H, W, C, OH, OW)
int usot_groupdw_multi_lp(void *stream, const usot_groupdw_desc *d, int nseg, int out_dtype)
    LAUNCH(usot_groupdw_multi_lp, arr(d, nseg), nseg, out_dtype)
int usot_groupdw_multi_dyn_f32(void *stream, const usot_groupdw_desc *d, int nseg, const int32_t *last_count)
    LAUNCH(usot_groupdw_multi_dyn_f32, arr(d, nseg), nseg, last_count)
int usot_conf_fusion_reduce_lp(void *stream, const void *cv, int in_dtype, void *out, int B, int M, int P, int C, int out_dtype)
    LAUNCH(usot_conf_fusion_reduce_lp, cv, in_dtype, out, B, M, P, C, out_dtype)
int usot_conf_fusion_reduce_map_f32(void *stream, const float *cv, float *out, int B, int M, int P, int C, const int32_t *map)
    LAUNCH(usot_conf_fusion_reduce_map_f32, cv, out, B, M, P, C, map)
int usot_prroi_pool_forward_f32(void *stream, const float *feat, const float *rois, float *out, int R, int C, int H, int W, int PH,
                                int PW, float scale, int64_t f_sb, int64_t f_sc, int64_t f_sh, int64_t f_sw, int64_t o_sr,
                                int64_t o_sc, int64_t o_sh, int64_t o_sw)
    LAUNCH(usot_prroi_pool_forward_f32, feat, rois, out, R, C, H, W, PH, PW, scale, f_sb, f_sc, f_sh, f_sw, o_sr, o_sc, o_sh, o_sw)
int usot_permute4_f32(void *stream, const float *src, float *dst, int D0, int D1, int D2, int D3, int64_t s0, int64_t s1, int64_t s2,
                      int64_t s3)
    LAUNCH(usot_permute4_f32, src, dst, D0, D1, D2, D3, s0, s1, s2, s3)
int usot_decode_dev_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox, const double *window, double *out,
                        int S, int instance_size, int stride, float ratio, double penalty_k, double window_influence,
                        const double *tsz_dev, float *roi_out)
    LAUNCH(usot_decode_dev_f32, cls, cls_mem, bbox, window, out, S, instance_size, stride, ratio, penalty_k, window_influence, tsz_dev,
           roi_out)
int usot_rows_copy_f32(void *stream, const float *src, const int32_t *idx_dev, float *dst, int n_rows, int row_len, int scatter)
    LAUNCH(usot_rows_copy_f32, src, idx_dev, dst, n_rows, row_len, scatter)
int usot_rows_copy_multi_f32(void *stream, int nseg, const float *const *src, const int32_t *idx_dev, float *const *dst, int n_rows,
                             const int32_t *row_len, int scatter, int32_t *stash_next)
    LAUNCH(usot_rows_copy_multi_f32, nseg, arr(src, 4), idx_dev, arr(dst, 4), n_rows, arr(row_len, 4), scatter, stash_next)
int usot_rows_append_gather_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos)
    LAUNCH(usot_rows_append_gather_f32, arr(fresh, 4), arr(bank, 4), arr(picked, 3), arr(row_len, 4), idx_dev, n_pick, slot_pos)
int usot_rows_append_gather_dedupe_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                       const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos, int32_t *mem_map)
    LAUNCH(usot_rows_append_gather_dedupe_f32, arr(fresh, 4), arr(bank, 4), arr(picked, 3), arr(row_len, 4), idx_dev, n_pick, slot_pos,
           mem_map)
int usot_decode_batch_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox, const double *window, double *out,
                          int B, int S, int instance_size, int stride, float ratio, double penalty_k, double window_influence,
                          const void *ctl, float *roi_out)
    LAUNCH(usot_decode_batch_f32, cls, cls_mem, bbox, window, out, B, S, instance_size, stride, ratio, penalty_k, window_influence, ctl,
           roi_out)
int usot_rows_append_gather_batch_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                      const int32_t *row_len, const void *ctl, int B, int n_pick, int bank_rows)
    LAUNCH(usot_rows_append_gather_batch_f32, arr(fresh, 4), arr(bank, 4), arr(picked, 3), arr(row_len, 4), ctl, B, n_pick, bank_rows)
int usot_crop_resize_batch_u8_f32(void *stream, const void *ctl, float *out, int B, int S)
    LAUNCH(usot_crop_resize_batch_u8_f32, ctl, out, B, S)
#undef LAUNCH

}  // extern "C"

// ------------------------------------------------------------------ recognisable arguments
static int g_seq = 100;
static int g_ptr = 0;
static int I(void) { return ++g_seq; }
static float F(void) { return (float)++g_seq + 0.5f; }
static double D(void) { return (double)++g_seq + 0.25; }
static void *P(void) { return arena + 8 * ++g_ptr; }
static float *PF(void) { return (float *)P(); }
static int32_t *PI(void) { return (int32_t *)P(); }
static double *PD(void) { return (double *)P(); }

// everything handed to an adder by pointer lives in a heap block that main() scribbles and frees before the plan runs
static std::vector<std::pair<void *, size_t>> g_blocks;
template <class T> static T *heap(int n = 1)
{
    T *p = (T *)calloc(n, sizeof(T));
    if (!p) abort();
    g_blocks.push_back({p, n * sizeof(T)});
    return p;
}
static void release(void)
{
    for (auto &b : g_blocks) {
        memset(b.first, 0xEE, b.second);
        free(b.first);
    }
    g_blocks.clear();
}

static usot_conv_desc *conv(int n = 1)
{
    usot_conv_desc *d = heap<usot_conv_desc>(n);
    for (int i = 0; i < n; ++i) {
        usot_conv_desc &c = d[i];
        c.x = PF(); c.w = PF(); c.bias = PF(); c.res = PF(); c.y = PF(); c.ws = PF();
        c.N = I(); c.H = I(); c.W = I(); c.Cin = I(); c.OH = I(); c.OW = I(); c.Cout = I();
        c.KH = I(); c.KW = I(); c.stride = I(); c.pad_h = I(); c.pad_w = I(); c.dil_h = I(); c.dil_w = I();
        c.y_cstride = I(); c.y_coff = I(); c.res_cstride = I(); c.res_coff = I(); c.y_nchw = I();
        c.act = I(); c.act2 = I(); c.act_split = I(); c.groups = I();
        c.x_gs = I(); c.w_gs = I(); c.b_gs = I(); c.y_gs = I(); c.r_gs = I();
        c.ksplit = I(); c.tile = I(); c.w_frag = I(); c.defer = I();
        c.w_scale = PF(); c.x_split = I(); c.y_split = I(); c.ovf = PI(); c.n_dyn = PI(); c.n_first = I();
    }
    return d;
}

static usot_pw_pair_desc *pair(void)
{
    usot_pw_pair_desc *d = heap<usot_pw_pair_desc>();
    d->t2 = P(); d->w3p = P(); d->res = P(); d->w1 = P(); d->b3 = PF(); d->b1 = PF(); d->y = P(); d->t = P();
    d->M = I(); d->CM = I(); d->CO = I(); d->CN = I(); d->act2 = I();
    d->ws = P(); d->t2_parts = I(); d->res_parts = I(); d->t2_bias = PF(); d->res_bias = PF(); d->ovf = PI();
    return d;
}

static usot_bneck_desc *bneck(void)
{
    usot_bneck_desc *d = heap<usot_bneck_desc>();
    d->x = P(); d->w1 = P(); d->w2 = P(); d->w3c = P(); d->wn = P();
    d->b1 = PF(); d->b2 = PF(); d->b3c = PF(); d->bn = PF(); d->y = P(); d->t = P();
    d->N = I(); d->H = I(); d->W = I();
    return d;
}

static usot_groupdw_desc *gdw(int n = 1)
{
    usot_groupdw_desc *d = heap<usot_groupdw_desc>(n);
    for (int i = 0; i < n; ++i) {
        usot_groupdw_desc &g = d[i];
        for (int b = 0; b < 3; ++b) {
            g.x[b] = PF(); g.z[b] = PF(); g.hk[b] = I(); g.wk[b] = I();
            g.x_cs[b] = I(); g.x_co[b] = I(); g.z_cs[b] = I(); g.z_co[b] = I(); g.wsm[b] = F();
        }
        g.out = PF(); g.S = I(); g.x_rep = I(); g.OH = I(); g.OW = I(); g.C = I(); g.cols_per_thread = I();
    }
    return d;
}

static const float **srcs(int n)
{
    const float **a = heap<const float *>(n);
    for (int i = 0; i < n; ++i) a[i] = PF();
    return a;
}
static float **dsts(int n)
{
    float **a = heap<float *>(n);
    for (int i = 0; i < n; ++i) a[i] = PF();
    return a;
}
static int32_t *lens(int n, int mul = 1)
{
    int32_t *a = heap<int32_t>(n);
    for (int i = 0; i < n; ++i) a[i] = mul * I();
    return a;
}

// ------------------------------------------------------------------ the script
static void *plan;

// A call whose arguments are evaluated left to right (a braced initialiser guarantees it; a plain call does not): the generators
// above then hand out the same values whatever the compiler.
struct Call {
    int rc;
    template <class F, class... A> Call(F f, A... a) : rc(f(a...)) {}
};
// an accepted add: status and the plan's new size
#define ACC(...) do { const int rc_ = Call{__VA_ARGS__}.rc; printf("+ %s -> %d size %d\n", #__VA_ARGS__, rc_, usot_plan_size(plan)); } while (0)
// a rejected add: status, and that the plan did not grow
#define REJ(...) do { const int n_ = usot_plan_size(plan); const int rc_ = Call{__VA_ARGS__}.rc; \
                      printf("- %s -> %d size %s\n", #__VA_ARGS__, rc_, usot_plan_size(plan) == n_ ? "unchanged" : "MOVED"); } while (0)

static void convs(void)
{
    usot_conv_desc *c1 = conv(), *c4 = conv(4), *c2 = conv(2), *lp = conv(), *bf = conv(), *t3 = conv(3), *t1 = conv();
    ACC(usot_plan_add_conv, plan, c1);
    ACC(usot_plan_add_conv_batch, plan, c1, 1);
    ACC(usot_plan_add_conv_batch, plan, c2, 2);
    ACC(usot_plan_add_conv_batch, plan, c4, 4);
    REJ(usot_plan_add_conv, plan, nullptr);
    REJ(usot_plan_add_conv, nullptr, c1);
    REJ(usot_plan_add_conv_batch, plan, nullptr, 1);
    REJ(usot_plan_add_conv_batch, plan, c4, 0);
    REJ(usot_plan_add_conv_batch, plan, c4, 5);
    REJ(usot_plan_add_conv_batch, nullptr, c4, 5);
    REJ(usot_plan_add_conv_batch, nullptr, c4, 4);
    ACC(usot_plan_add_conv_lp, plan, lp, I(), I());
    ACC(usot_plan_add_conv_bf16, plan, bf);
    REJ(usot_plan_add_conv_lp, plan, nullptr, 0, 0);
    REJ(usot_plan_add_conv_lp, nullptr, lp, 0, 0);
    REJ(usot_plan_add_conv_bf16, plan, nullptr);
    REJ(usot_plan_add_conv_bf16, nullptr, bf);
    ACC(usot_plan_add_thin_conv, plan, t1, 1);
    ACC(usot_plan_add_thin_conv, plan, t3, 3);
    REJ(usot_plan_add_thin_conv, plan, nullptr, 1);
    REJ(usot_plan_add_thin_conv, plan, t3, 0);
    REJ(usot_plan_add_thin_conv, plan, t3, 5);
    REJ(usot_plan_add_thin_conv, nullptr, t3, 3);
}

static void pairs(void)
{
    usot_pw_pair_desc *d = pair();
    for (int dtype = 0; dtype <= 3; ++dtype) {
        printf("# dtype %d\n", dtype);
        ACC(usot_plan_add_pw_pair, plan, d, dtype);
    }
    REJ(usot_plan_add_pw_pair, plan, nullptr, 0);
    REJ(usot_plan_add_pw_pair, nullptr, d, 0);
    g_supported = 0;
    for (int dtype = 0; dtype <= 3; ++dtype) {
        printf("# dtype %d\n", dtype);
        REJ(usot_plan_add_pw_pair, plan, d, dtype);
    }
    g_supported = 1;
    usot_pw_pair_desc *wide = pair();       // the channel-sliced (256, 1024, 256) fp32 pair: workspace required
    wide->CM = 256;
    for (int dtype = 0; dtype <= 3; ++dtype) {
        printf("# dtype %d\n", dtype);
        ACC(usot_plan_add_pw_pair, plan, wide, dtype);
    }
    g_ws_floats = 0;
    REJ(usot_plan_add_pw_pair, plan, wide, 2);
    REJ(usot_plan_add_pw_pair, plan, wide, 3);
    ACC(usot_plan_add_pw_pair, plan, wide, 1);
    g_ws_floats = 7;
    wide->ws = NULL;
    REJ(usot_plan_add_pw_pair, plan, wide, 2);
    REJ(usot_plan_add_pw_pair, plan, wide, 3);
    REJ(usot_plan_add_pw_pair, nullptr, wide, 3);
    ACC(usot_plan_add_pw_pair, plan, wide, 0);

    usot_pw_pair_desc *pp = pair();
    ACC(usot_plan_add_pw_panel_pair, plan, pp, 0);
    ACC(usot_plan_add_pw_panel_pair, plan, pp, 1);
    REJ(usot_plan_add_pw_panel_pair, plan, nullptr, 0);
    REJ(usot_plan_add_pw_panel_pair, plan, pp, 2);
    REJ(usot_plan_add_pw_panel_pair, plan, pp, -1);
    REJ(usot_plan_add_pw_panel_pair, nullptr, pp, 0);
    g_supported = 0;
    REJ(usot_plan_add_pw_panel_pair, plan, pp, 0);
    g_supported = 1;

    usot_conv_desc *c2 = conv();
    usot_pw_pair_desc *cp = pair();
    ACC(usot_plan_add_conv_pw, plan, c2, P(), PF(), P(), P(), 1);
    REJ(usot_plan_add_conv_pw, plan, nullptr, P(), PF(), P(), P(), 0);
    REJ(usot_plan_add_conv_pw, plan, c2, P(), PF(), P(), P(), 2);
    REJ(usot_plan_add_conv_pw, plan, c2, P(), PF(), P(), P(), -1);
    REJ(usot_plan_add_conv_pw, nullptr, c2, P(), PF(), P(), P(), 0);
    ACC(usot_plan_add_conv_pw_pair, plan, c2, cp, 1);
    REJ(usot_plan_add_conv_pw_pair, plan, nullptr, cp, 0);
    REJ(usot_plan_add_conv_pw_pair, plan, c2, nullptr, 0);
    REJ(usot_plan_add_conv_pw_pair, plan, c2, cp, 2);
    REJ(usot_plan_add_conv_pw_pair, plan, c2, cp, -1);
    REJ(usot_plan_add_conv_pw_pair, nullptr, c2, cp, 0);
    ACC(usot_plan_add_conv_pw_ov, plan, c2, cp, 1, P());
    REJ(usot_plan_add_conv_pw_ov, plan, nullptr, cp, 0, P());
    REJ(usot_plan_add_conv_pw_ov, plan, c2, nullptr, 0, P());
    REJ(usot_plan_add_conv_pw_ov, plan, c2, cp, 0, nullptr);
    REJ(usot_plan_add_conv_pw_ov, plan, c2, cp, 2, P());
    REJ(usot_plan_add_conv_pw_ov, plan, c2, cp, -1, P());
    REJ(usot_plan_add_conv_pw_ov, nullptr, c2, cp, 0, P());
    g_supported = 0;
    REJ(usot_plan_add_conv_pw, plan, c2, P(), PF(), P(), P(), 0);
    REJ(usot_plan_add_conv_pw_pair, plan, c2, cp, 0);
    REJ(usot_plan_add_conv_pw_ov, plan, c2, cp, 0, P());
    g_supported = 1;

    usot_pw_pair_desc *tr = pair();
    ACC(usot_plan_add_pw_triple, plan, PF(), PF(), PF(), tr, I(), I(), I(), I(), I(), I(), I(), I(), I(), I());
    REJ(usot_plan_add_pw_triple, plan, PF(), PF(), PF(), nullptr, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10);
    REJ(usot_plan_add_pw_triple, nullptr, PF(), PF(), PF(), tr, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10);
    g_supported = 0;
    REJ(usot_plan_add_pw_triple, plan, PF(), PF(), PF(), tr, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10);
    g_supported = 1;
}

static void flat(void)      // adders whose arguments are all scalars and device pointers
{
    ACC(usot_plan_add_pw_single, plan, PF(), PF(), PF(), PF(), PF(), I(), I(), I(), I());
    ACC(usot_plan_add_conv3x3_halo, plan, P(), P(), PF(), P(), I(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_conv_kstream, plan, P(), P(), PF(), P(), I(), I(), I(), I(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_pw_kstream, plan, P(), P(), PF(), P(), 5000000000L + I(), I(), I(), I(), I());
    ACC(usot_plan_add_pw_panel, plan, P(), P(), PF(), P(), P(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_stream_conv3x3, plan, PF(), PF(), PF(), PF(), PF(), I(), I(), I(), I(), I(), I(), I(), I(), I(), I(), I(), I());
    REJ(usot_plan_add_pw_single, nullptr, PF(), PF(), PF(), PF(), PF(), 1, 2, 3, 4);
    REJ(usot_plan_add_conv3x3_halo, nullptr, P(), P(), PF(), P(), 1, 2, 3, 4, 5, 6, 7);
    REJ(usot_plan_add_conv_kstream, nullptr, P(), P(), PF(), P(), 1, 2, 3, 4, 5, 6, 7, 8, 9, 10);
    REJ(usot_plan_add_pw_kstream, nullptr, P(), P(), PF(), P(), 1L, 2, 3, 4, 5);
    REJ(usot_plan_add_pw_panel, nullptr, P(), P(), PF(), P(), P(), 1, 2, 3, 4, 5);
    REJ(usot_plan_add_stream_conv3x3, nullptr, PF(), PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12);
    g_supported = 0;
    REJ(usot_plan_add_pw_single, plan, PF(), PF(), PF(), PF(), PF(), 1, 2, 3, 4);
    REJ(usot_plan_add_conv3x3_halo, plan, P(), P(), PF(), P(), 1, 2, 3, 4, 5, 6, 7);
    REJ(usot_plan_add_conv_kstream, plan, P(), P(), PF(), P(), 1, 2, 3, 4, 5, 6, 7, 8, 9, 10);
    REJ(usot_plan_add_pw_kstream, plan, P(), P(), PF(), P(), 1L, 2, 3, 4, 5);
    REJ(usot_plan_add_pw_panel, plan, P(), P(), PF(), P(), P(), 1, 2, 3, 4, 5);
    REJ(usot_plan_add_stream_conv3x3, plan, PF(), PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12);
    REJ(usot_plan_add_pw_single, nullptr, PF(), PF(), PF(), PF(), PF(), 1, 2, 3, 4);
    g_supported = 1;

    ACC(usot_plan_add_cvt_lp, plan, PF(), P(), 6000000000L + I(), I());
    ACC(usot_plan_add_cvt_bf16, plan, PF(), P(), 7000000000L + I());
    ACC(usot_plan_add_maxpool_lp, plan, P(), P(), I(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_maxpool_bf16, plan, P(), P(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_maxpool, plan, PF(), PF(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_stem_pool_lp, plan, PF(), P(), PF(), P(), I(), I(), I(), I(), I(), I(), I(), I(), F(), F(), F());
    ACC(usot_plan_add_stem_pool, plan, PF(), PF(), PF(), PF(), I(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_stem_pool_ind, plan, PF(), PF(), PF(), PF(), I(), I(), I(), I(), I(), I(), I(), PI());
    ACC(usot_plan_add_stem_pool_mu, plan, PF(), PF(), PF(), PF(), I(), I(), I(), I(), I(), I(), I(), PI(), F(), F(), F());
    ACC(usot_plan_add_stem, plan, PF(), PF(), PF(), PF(), I(), I(), I(), I(), I());
    ACC(usot_plan_add_stem_mu, plan, PF(), PF(), PF(), PF(), I(), I(), I(), I(), I(), F(), F(), F());
    ACC(usot_plan_add_prroi, plan, PF(), PF(), PF(), I(), I(), I(), I(), I(), I(), F(), 8000000000L + I(), 8000000000L + I(),
                            8000000000L + I(), 8000000000L + I(), 8000000000L + I(), 8000000000L + I(), 8000000000L + I(),
                            8000000000L + I());
    ACC(usot_plan_add_permute, plan, PF(), PF(), I(), I(), I(), I(), 9000000000L + I(), 9000000000L + I(), 9000000000L + I(),
                              9000000000L + I());
    ACC(usot_plan_add_decode, plan, PF(), PF(), PF(), PD(), PD(), I(), I(), I(), F(), D(), D(), PD(), PF());
    ACC(usot_plan_add_decode, plan, PF(), PF(), PF(), PD(), PD(), I(), I(), I(), F(), D(), D(), PD(), nullptr);
    ACC(usot_plan_add_rows_copy, plan, PF(), PI(), PF(), I(), I(), I());
    ACC(usot_plan_add_conf_reduce, plan, PF(), PF(), I(), I(), I(), I());
    ACC(usot_plan_add_conf_reduce_map, plan, PF(), PF(), I(), I(), I(), I(), PI());
    ACC(usot_plan_add_conf_reduce_map, plan, PF(), PF(), I(), I(), I(), I(), nullptr);
    ACC(usot_plan_add_conf_reduce_lp, plan, P(), 0, P(), I(), I(), I(), I(), 1);
    ACC(usot_plan_add_conf_reduce_lp, plan, P(), 2, P(), I(), I(), I(), I(), 2);
    REJ(usot_plan_add_conf_reduce_lp, plan, P(), 0, P(), 1, 2, 3, 4, 0);
    REJ(usot_plan_add_conf_reduce_lp, plan, P(), 0, P(), 1, 2, 3, 4, 3);
    REJ(usot_plan_add_conf_reduce_lp, plan, P(), -1, P(), 1, 2, 3, 4, 1);
    REJ(usot_plan_add_conf_reduce_lp, plan, P(), 3, P(), 1, 2, 3, 4, 1);
    REJ(usot_plan_add_conf_reduce_lp, nullptr, P(), 3, P(), 1, 2, 3, 4, 1);
    REJ(usot_plan_add_conf_reduce_lp, nullptr, P(), 1, P(), 1, 2, 3, 4, 1);
    REJ(usot_plan_add_cvt_lp, nullptr, PF(), P(), 1L, 0);
    REJ(usot_plan_add_cvt_bf16, nullptr, PF(), P(), 1L);
    REJ(usot_plan_add_maxpool_lp, nullptr, P(), P(), 1, 2, 3, 4, 5, 6, 0);
    REJ(usot_plan_add_maxpool_bf16, nullptr, P(), P(), 1, 2, 3, 4, 5, 6);
    REJ(usot_plan_add_maxpool, nullptr, PF(), PF(), 1, 2, 3, 4, 5, 6);
    REJ(usot_plan_add_stem_pool_lp, nullptr, PF(), P(), PF(), P(), 1, 2, 3, 4, 5, 6, 7, 0, 1.f, 2.f, 3.f);
    REJ(usot_plan_add_stem_pool, nullptr, PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 7);
    REJ(usot_plan_add_stem_pool_ind, nullptr, PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 7, PI());
    REJ(usot_plan_add_stem_pool_mu, nullptr, PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 7, PI(), 1.f, 2.f, 3.f);
    REJ(usot_plan_add_stem, nullptr, PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5);
    REJ(usot_plan_add_stem_mu, nullptr, PF(), PF(), PF(), PF(), 1, 2, 3, 4, 5, 1.f, 2.f, 3.f);
    REJ(usot_plan_add_prroi, nullptr, PF(), PF(), PF(), 1, 2, 3, 4, 5, 6, 1.f, 1L, 2L, 3L, 4L, 5L, 6L, 7L, 8L);
    REJ(usot_plan_add_permute, nullptr, PF(), PF(), 1, 2, 3, 4, 1L, 2L, 3L, 4L);
    REJ(usot_plan_add_decode, nullptr, PF(), PF(), PF(), PD(), PD(), 1, 2, 3, 1.f, 2.0, 3.0, PD(), PF());
    REJ(usot_plan_add_rows_copy, nullptr, PF(), PI(), PF(), 1, 2, 3);
    REJ(usot_plan_add_conf_reduce, nullptr, PF(), PF(), 1, 2, 3, 4);
    REJ(usot_plan_add_conf_reduce_map, nullptr, PF(), PF(), 1, 2, 3, 4, PI());
}

static void bnecks(void)
{
    usot_bneck_desc *b = bneck();
    ACC(usot_plan_add_bneck_first, plan, b, 0);
    ACC(usot_plan_add_bneck_first, plan, b, 1);
    ACC(usot_plan_add_bneck_tail, plan, b, I(), 1);
    REJ(usot_plan_add_bneck_first, plan, nullptr, 0);
    REJ(usot_plan_add_bneck_first, plan, b, 2);
    REJ(usot_plan_add_bneck_first, plan, b, -1);
    REJ(usot_plan_add_bneck_first, nullptr, b, 0);
    REJ(usot_plan_add_bneck_tail, plan, nullptr, 64, 0);
    REJ(usot_plan_add_bneck_tail, plan, b, 64, 2);
    REJ(usot_plan_add_bneck_tail, plan, b, 64, -1);
    REJ(usot_plan_add_bneck_tail, nullptr, b, 64, 0);
    g_supported = 0;
    REJ(usot_plan_add_bneck_tail, plan, b, 64, 0);
    g_supported = 1;
}

static void groupdws(void)
{
    usot_groupdw_desc *g1 = gdw(), *g3 = gdw(3), *g2 = gdw(2);
    ACC(usot_plan_add_groupdw, plan, g1);
    ACC(usot_plan_add_groupdw_multi, plan, g3, 3);
    ACC(usot_plan_add_groupdw_multi_dyn, plan, g2, 2, PI());
    ACC(usot_plan_add_groupdw_multi_dyn, plan, g2, 1, nullptr);
    ACC(usot_plan_add_groupdw_multi_lp, plan, g3, 3, 1);
    ACC(usot_plan_add_groupdw_multi_lp, plan, g2, 2, 2);
    REJ(usot_plan_add_groupdw, plan, nullptr);
    REJ(usot_plan_add_groupdw, nullptr, g1);
    REJ(usot_plan_add_groupdw_multi, plan, nullptr, 1);
    REJ(usot_plan_add_groupdw_multi, plan, g3, 0);
    REJ(usot_plan_add_groupdw_multi, plan, g3, 4);
    REJ(usot_plan_add_groupdw_multi, nullptr, g3, 3);
    REJ(usot_plan_add_groupdw_multi_dyn, plan, nullptr, 1, PI());
    REJ(usot_plan_add_groupdw_multi_dyn, plan, g3, 0, PI());
    REJ(usot_plan_add_groupdw_multi_dyn, plan, g3, 4, PI());
    REJ(usot_plan_add_groupdw_multi_dyn, nullptr, g3, 3, PI());
    REJ(usot_plan_add_groupdw_multi_dyn, nullptr, g3, 4, PI());
    REJ(usot_plan_add_groupdw_multi_lp, plan, nullptr, 1, 1);
    REJ(usot_plan_add_groupdw_multi_lp, plan, g3, 0, 1);
    REJ(usot_plan_add_groupdw_multi_lp, plan, g3, 4, 1);
    REJ(usot_plan_add_groupdw_multi_lp, plan, g3, 3, 0);
    REJ(usot_plan_add_groupdw_multi_lp, plan, g3, 3, 3);
    REJ(usot_plan_add_groupdw_multi_lp, nullptr, g3, 3, 1);
}

static void rows(void)
{
    const float **src = srcs(4);
    float **dst = dsts(4);
    int32_t *len = lens(4);
    ACC(usot_plan_add_rows_copy_multi, plan, 4, src, PI(), dst, I(), len, I(), PI());
    ACC(usot_plan_add_rows_copy_multi, plan, 2, src, PI(), dst, I(), len, I(), nullptr);
    REJ(usot_plan_add_rows_copy_multi, plan, 0, src, PI(), dst, 1, len, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, plan, 5, src, PI(), dst, 1, len, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, plan, 4, nullptr, PI(), dst, 1, len, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, plan, 4, src, PI(), nullptr, 1, len, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, plan, 4, src, PI(), dst, 1, nullptr, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, nullptr, 4, src, PI(), dst, 1, len, 0, nullptr);
    REJ(usot_plan_add_rows_copy_multi, nullptr, 5, src, PI(), dst, 1, len, 0, nullptr);

    const float **fresh = srcs(4);
    float **bank = dsts(4), **picked = dsts(3);
    int32_t *rl = lens(4);
    int32_t *idx = PI(), *map = PI();
    ACC(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, idx, 32, 0);
    ACC(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, PI(), 1, I());
    REJ(usot_plan_add_rows_append_gather, plan, nullptr, bank, picked, rl, idx, 3, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, nullptr, picked, rl, idx, 3, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, nullptr, rl, idx, 3, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, nullptr, idx, 3, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, nullptr, 3, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, idx, 0, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, idx, 33, 1);
    REJ(usot_plan_add_rows_append_gather, plan, fresh, bank, picked, rl, idx, 3, -1);
    REJ(usot_plan_add_rows_append_gather, nullptr, fresh, bank, picked, rl, idx, 3, 1);
    REJ(usot_plan_add_rows_append_gather, nullptr, fresh, bank, picked, rl, idx, 33, 1);
    ACC(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, PI(), I() % 32 + 1, I(), map);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 3, 1, nullptr);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 3, 1, (int32_t *)((char *)map + 1));
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 3, 1, (int32_t *)((char *)map + 2));
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, nullptr, bank, picked, rl, idx, 3, 1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, nullptr, 3, 1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 0, 1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 33, 1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, plan, fresh, bank, picked, rl, idx, 3, -1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, nullptr, fresh, bank, picked, rl, idx, 3, 1, map);
    REJ(usot_plan_add_rows_append_gather_dedupe, nullptr, fresh, bank, picked, rl, idx, 3, 1, nullptr);
}

static void multitrack(void)
{
    const float *cls = PF(), *cm = PF(), *bbox = PF();
    const double *win = PD();
    double *out = PD();
    const void *ctl = P();
    float *roi = PF();
    ACC(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 65535, 32, I(), I(), F(), D(), D(), ctl, roi);
    ACC(usot_plan_add_decode_batch, plan, PF(), PF(), PF(), PD(), PD(), 1, 1, I(), I(), F(), D(), D(), P(), PF());
    REJ(usot_plan_add_decode_batch, nullptr, cls, cm, bbox, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, nullptr, cm, bbox, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, nullptr, bbox, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, nullptr, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, nullptr, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, nullptr, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, nullptr, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 2, 25, 255, 8, 1.f, 2.0, 3.0, ctl, nullptr);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 0, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 65536, 25, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 2, 0, 255, 8, 1.f, 2.0, 3.0, ctl, roi);
    REJ(usot_plan_add_decode_batch, plan, cls, cm, bbox, win, out, 2, 33, 255, 8, 1.f, 2.0, 3.0, ctl, roi);

    const float **fresh = srcs(4);
    float **bank = dsts(4), **picked = dsts(3);
    int32_t *rl = lens(4, 4);
    ACC(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 65535, 32, I());
    ACC(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, P(), 1, 1, 1);
    REJ(usot_plan_add_rows_append_gather_batch, nullptr, fresh, bank, picked, rl, ctl, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, nullptr, bank, picked, rl, ctl, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, nullptr, picked, rl, ctl, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, nullptr, rl, ctl, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, nullptr, ctl, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, nullptr, 2, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 0, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 65536, 7, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 0, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 33, 16);
    REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 0);
    for (int q = 0; q < 4; ++q) {       // one bad element of each array at a time
        printf("# fresh[%d] = NULL\n", q);
        const float *f = fresh[q]; fresh[q] = NULL;
        REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
        fresh[q] = f;
        printf("# bank[%d] = NULL\n", q);
        float *b = bank[q]; bank[q] = NULL;
        REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
        bank[q] = b;
        const int32_t l = rl[q];
        printf("# row_len[%d] = 0, then -4, then not a multiple of 4\n", q);
        rl[q] = 0;
        REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
        rl[q] = -4;
        REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
        rl[q] = l + 2;
        REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
        rl[q] = l;
        if (q < 3) {
            printf("# picked[%d] = NULL\n", q);
            float *p = picked[q]; picked[q] = NULL;
            REJ(usot_plan_add_rows_append_gather_batch, plan, fresh, bank, picked, rl, ctl, 2, 7, 16);
            picked[q] = p;
        }
    }

    ACC(usot_plan_add_crop_resize_batch, plan, ctl, PF(), 65535, 4096);
    ACC(usot_plan_add_crop_resize_batch, plan, P(), PF(), 1, 1);
    REJ(usot_plan_add_crop_resize_batch, nullptr, ctl, roi, 2, 255);
    REJ(usot_plan_add_crop_resize_batch, plan, nullptr, roi, 2, 255);
    REJ(usot_plan_add_crop_resize_batch, plan, ctl, nullptr, 2, 255);
    REJ(usot_plan_add_crop_resize_batch, plan, ctl, roi, 0, 255);
    REJ(usot_plan_add_crop_resize_batch, plan, ctl, roi, 65536, 255);
    REJ(usot_plan_add_crop_resize_batch, plan, ctl, roi, 2, 0);
    REJ(usot_plan_add_crop_resize_batch, plan, ctl, roi, 2, 4097);
}

static void lanes(void)
{
    ACC(usot_plan_fork, plan, 1);
    ACC(usot_plan_add_rows_copy, plan, PF(), PI(), PF(), I(), I(), I());
    ACC(usot_plan_fork, plan, 3);
    ACC(usot_plan_add_maxpool, plan, PF(), PF(), I(), I(), I(), I(), I(), I());
    ACC(usot_plan_fork, plan, 0);
    ACC(usot_plan_add_rows_copy, plan, PF(), PI(), PF(), I(), I(), I());
    ACC(usot_plan_join, plan, 1);
    ACC(usot_plan_join, plan, 3);
    ACC(usot_plan_join, plan, 0);
    REJ(usot_plan_fork, plan, -1);
    REJ(usot_plan_fork, plan, 4);
    REJ(usot_plan_join, plan, -1);
    REJ(usot_plan_join, plan, 4);
    REJ(usot_plan_fork, nullptr, 1);
    REJ(usot_plan_join, nullptr, 1);
    ACC(usot_plan_add_rows_copy, plan, PF(), PI(), PF(), I(), I(), I());
}

int main(void)
{
    void *const first = usot_plan_create();
    void *const stream = P();
    plan = first;
    printf("empty plan: size %d, run %d, op_info %d\n", usot_plan_size(plan), usot_plan_run(plan, stream), usot_plan_op_info(plan, 0, NULL));
    printf("no plan: size %d, run %d\n", usot_plan_size(NULL), usot_plan_run(NULL, stream));
    convs();
    pairs();
    flat();
    bnecks();
    groupdws();
    rows();
    multitrack();
    lanes();
    release();      // the plan owns everything it needs from here on

    const int n = usot_plan_size(plan);
    printf("plan size %d\n", n);
    for (int i = -1; i <= n; ++i) {
        int info[4] = {-7, -7, -7, -7};
        const int rc = usot_plan_op_info(plan, i, info);
        printf("op %d: rc %d info %d %d %d %d\n", i, rc, info[0], info[1], info[2], info[3]);
        g_tile += 1;
    }
    for (int run = 0; run < 2; ++run) {
        g_calls = 0;
        const int rc = usot_plan_run(plan, stream);
        printf("run %d on", run);
        put(stream);
        printf(": rc %d after %d launches\n", rc, g_calls);
    }

    void *bad = usot_plan_create();      // the third launch fails: the run stops there with its code
    plan = bad;
    for (int i = 0; i < 5; ++i) ACC(usot_plan_add_rows_copy, plan, PF(), PI(), PF(), I(), I(), I());
    g_calls = 0;
    g_fail_at = 3;
    int rc = usot_plan_run(bad, stream);
    printf("failing run: rc %d after %d launches\n", rc, g_calls);
    g_fail_at = 0;
    g_calls = 0;
    rc = usot_plan_run(bad, stream);
    printf("same plan again: rc %d after %d launches\n", rc, g_calls);
    usot_plan_destroy(first);
    usot_plan_destroy(bad);
    usot_plan_destroy(NULL);
    return 0;
}
