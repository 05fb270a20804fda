// The two head operators that had no gradient: Conf_Fusion on separate conf / value maps (connect.py:123-144) and the box epilogue
// exp(adjust * bbox_pred + bias) (connect.py:236-237), forward and backward, fp32 on NHWC maps; usot_conf_fusion_desc and
// usot_box_exp_desc in usot_hip.h state the arithmetic.  Everything here is bandwidth.
//
// Conf_Fusion: one lane per (b, p, c/4), a f32x4 of four channels, as in conf_fusion_reduce_kernel (head_ops.hip); one lane per
// thread, the grid is ceil(lanes / 256) workgroups (no grid-stride loop).  A lane walks the M maps of its batch element twice
// - S (and out), then out or the gradients; the second walk hits in L1 / L2 - and recomputes e_m = exp(clamp(conf_m)) in each
// walk through cf_e(), so the weights of the backward pass are the forward's, bit for bit.  The backward pass re-forms `out`
// in float64 (conf_fusion_bwd_f32 says why).
//
// Box-exp: one thread per row of four channels.  The backward kernel leaves each workgroup's five sums (dbias[0..3], dadjust) of
// its BX_ROWS rows in ws[workgroup][5] with plain stores - a fixed tree over the 256 threads in LDS - and a second launch of one
// workgroup merges the partials: thread t adds partials t, t + 256, ... ascending in float64, then the same tree.  No atomics; the
// order depends on R alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <initializer_list>
#include "usot_hip.h"
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BX_ROWS = 256;           // rows per workgroup of the box-exp kernels: one per thread
constexpr int BX_SUMS = 5;             // dbias[0..3], dadjust

struct CfK {
    const float *conf, *value, *dout;
    float *out, *dconf, *dvalue;
    int M, P, C4;
    long lanes;
};

// e = exp(clamp(conf, -6, 4)); fminf / fmaxf keep a finite conf's value, so conf == 4 and conf == -6 go through unchanged
__device__ __forceinline__ f32x4 cf_e(f32x4 c)
{
    f32x4 e;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = expf(fminf(fmaxf(c[k], -6.f), 4.f));
    return e;
}

// S = sum_m e_m and out = sum_m (e_m / S) * value_m, both in m order: the reference's association (normalise, weight, add)
__device__ __forceinline__ f32x4 cf_sum(const CfK &p, long base, long ms)
{
    f32x4 S = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < p.M; ++m) S += cf_e(*(const f32x4 *)(p.conf + base + m * ms));
    return S;
}

__device__ __forceinline__ f32x4 cf_out(const CfK &p, long base, long ms, f32x4 S)
{
#pragma clang fp contract(off)
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < p.M; ++m) {
        const f32x4 e = cf_e(*(const f32x4 *)(p.conf + base + m * ms));
        const f32x4 v = *(const f32x4 *)(p.value + base + m * ms);
        out += (e / S) * v;
    }
    return out;
}

// lane -> element offset of its four channels in map 0 of its batch element, and in out / dout
__device__ __forceinline__ void cf_lane(const CfK &p, long idx, long &base, long &obase)
{
    const int c = (int)(idx % p.C4);
    const long bp = idx / p.C4;
    const int pix = (int)(bp % p.P);
    const long b = bp / p.P;
    base = ((b * p.M * p.P + pix) * p.C4 + c) * 4;
    obase = idx * 4;
}

__global__ __launch_bounds__(256) void conf_fusion_fwd_f32(const CfK p)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.lanes) return;
    long base, obase;
    cf_lane(p, idx, base, obase);
    const long ms = (long)p.P * p.C4 * 4;
    const f32x4 S = cf_sum(p, base, ms);
    *(f32x4 *)(p.out + obase) = cf_out(p, base, ms, S);
}

__global__ __launch_bounds__(256) void conf_fusion_bwd_f32(const CfK p)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.lanes) return;
    long base, obase;
    cf_lane(p, idx, base, obase);
    const long ms = (long)p.P * p.C4 * 4;
    // S as the forward forms it; for dconf also `out`, re-formed in float64 from the same e_m: where one weight dominates,
    // value_m - out = sum_k w_k (value_m - value_k) is far below an ulp of value_m times the roundings of a float32 `out`
    f32x4 S = {0.f, 0.f, 0.f, 0.f};
    usot_f64x4 den = {0., 0., 0., 0.}, num = {0., 0., 0., 0.};
    for (int m = 0; m < p.M; ++m) {
        const f32x4 e = cf_e(*(const f32x4 *)(p.conf + base + m * ms));
        S += e;
        if (p.dconf) {
            const usot_f64x4 e64 = __builtin_convertvector(e, usot_f64x4);
            den += e64;
            num += e64 * __builtin_convertvector(*(const f32x4 *)(p.value + base + m * ms), usot_f64x4);
        }
    }
    const usot_f64x4 out = num / den;
    const f32x4 g = *(const f32x4 *)(p.dout + obase);
    for (int m = 0; m < p.M; ++m) {
        const f32x4 c = *(const f32x4 *)(p.conf + base + m * ms);
        const f32x4 w = cf_e(c) / S;
        const f32x4 wg = w * g;
        if (p.dvalue) *(f32x4 *)(p.dvalue + base + m * ms) = wg;
        if (p.dconf) {
            const f32x4 v = *(const f32x4 *)(p.value + base + m * ms);
            f32x4 d = wg * __builtin_convertvector(__builtin_convertvector(v, usot_f64x4) - out, f32x4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!(c[k] >= -6.f && c[k] <= 4.f)) d[k] = 0.f;          // torch.clamp's gradient: the bounds are inside
            *(f32x4 *)(p.dconf + base + m * ms) = d;
        }
    }
}

struct BxK {
    const float *p, *adjust, *bias, *dy;
    float *y, *dp, *dadjust, *dbias, *ws;
    int R, parts;
};

// y of one row: the one place it is formed, an fma and expf per channel
__device__ __forceinline__ f32x4 bx_y(f32x4 v, float a, f32x4 b)
{
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = expf(fmaf(a, v[k], b[k]));
    return y;
}

__global__ __launch_bounds__(256) void box_exp_fwd_f32(const BxK p)
{
    const long r = (long)blockIdx.x * BX_ROWS + threadIdx.x;
    if (r >= p.R) return;
    const float a = p.adjust[0];
    const f32x4 b = *(const f32x4 *)p.bias;
    *(f32x4 *)(p.y + r * 4) = bx_y(*(const f32x4 *)(p.p + r * 4), a, b);
}

// sm[k][t], k < BX_SUMS: the 256 values of sum k -> sm[k][0], the same tree for every call
__device__ __forceinline__ void bx_tree(float (*sm)[256], int t)
{
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h)
#pragma unroll
            for (int k = 0; k < BX_SUMS; ++k) sm[k][t] += sm[k][t + h];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void box_exp_bwd_f32(const BxK p)
{
    __shared__ float sm[BX_SUMS][256];
    const int t = threadIdx.x;
    const long r = (long)blockIdx.x * BX_ROWS + t;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    float ga = 0.f;
    if (r < p.R) {
        const float a = p.adjust[0];
        const f32x4 b = *(const f32x4 *)p.bias;
        const f32x4 v = *(const f32x4 *)(p.p + r * 4);
        g = *(const f32x4 *)(p.dy + r * 4) * bx_y(v, a, b);
        if (p.dp) *(f32x4 *)(p.dp + r * 4) = a * g;
        ga = (g[0] * v[0] + g[1] * v[1]) + (g[2] * v[2] + g[3] * v[3]);
    }
    if (!p.ws) return;                   // dp alone: no reduction (uniform over the grid)
#pragma unroll
    for (int k = 0; k < 4; ++k) sm[k][t] = g[k];
    sm[4][t] = ga;
    bx_tree(sm, t);
    if (t < BX_SUMS) p.ws[(long)blockIdx.x * BX_SUMS + t] = sm[t][0];
}

__global__ __launch_bounds__(256) void box_exp_merge_f32(const BxK p)
{
    __shared__ double sm[BX_SUMS][256];
    const int t = threadIdx.x;
    double a[BX_SUMS] = {0., 0., 0., 0., 0.};
    for (int s = t; s < p.parts; s += 256)
#pragma unroll
        for (int k = 0; k < BX_SUMS; ++k) a[k] += (double)p.ws[(long)s * BX_SUMS + k];
#pragma unroll
    for (int k = 0; k < BX_SUMS; ++k) sm[k][t] = a[k];
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h)
#pragma unroll
            for (int k = 0; k < BX_SUMS; ++k) sm[k][t] += sm[k][t + h];
    }
    __syncthreads();
    if (t < 4 && p.dbias) p.dbias[t] = (float)sm[t][0];
    if (t == 4 && p.dadjust) p.dadjust[0] = (float)sm[4][0];
}

bool misaligned(std::initializer_list<const void *> ps)
{
    uintptr_t a = 0;
    for (const void *q : ps) a |= (uintptr_t)q;
    return (a & 15) != 0;
}

// lanes of a Conf_Fusion launch, or 0 for a geometry the launchers reject (the grid's x holds ceil(lanes / 256) workgroups)
long cf_lanes(const usot_conf_fusion_desc *d)
{
    if (!d || d->B < 1 || d->M < 1 || d->P < 1 || d->C < 4 || (d->C & 3)) return 0;
    const long lanes = (long)d->B * d->P * (d->C / 4);
    if ((lanes + 255) / 256 > 0x7fffffffL) return 0;
    if ((long)d->B * d->M > (1L << 62) / ((long)d->P * d->C)) return 0;
    return lanes;
}

void cf_fill(const usot_conf_fusion_desc *d, long lanes, CfK &p)
{
    p.conf = d->conf; p.value = d->value; p.dout = d->dout;
    p.out = d->out; p.dconf = d->dconf; p.dvalue = d->dvalue;
    p.M = d->M; p.P = d->P; p.C4 = d->C / 4; p.lanes = lanes;
}

int bx_geometry_ok(const usot_box_exp_desc *d) { return d && d->R >= 1 && d->C == 4; }
int bx_parts(const usot_box_exp_desc *d) { return (int)(((long)d->R + BX_ROWS - 1) / BX_ROWS); }

void bx_fill(const usot_box_exp_desc *d, BxK &p)
{
    p.p = d->p; p.adjust = d->adjust; p.bias = d->bias; p.dy = d->dy;
    p.y = d->y; p.dp = d->dp; p.dadjust = d->dadjust; p.dbias = d->dbias; p.ws = d->ws;
    p.R = d->R; p.parts = bx_parts(d);
}

}  // namespace

extern "C" int usot_conf_fusion_fwd_f32(void *stream, const usot_conf_fusion_desc *d)
{
    const long lanes = cf_lanes(d);
    if (!lanes || !d->conf || !d->value || !d->out) return USOT_EINVAL;
    if (misaligned({d->conf, d->value, d->out})) return USOT_EINVAL;
    CfK p;
    cf_fill(d, lanes, p);
    hipLaunchKernelGGL(conf_fusion_fwd_f32, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_conf_fusion_bwd_f32(void *stream, const usot_conf_fusion_desc *d)
{
    const long lanes = cf_lanes(d);
    if (!lanes || !d->conf || !d->dout || (d->dconf && !d->value)) return USOT_EINVAL;
    if (misaligned({d->conf, d->value, d->dout, d->dconf, d->dvalue})) return USOT_EINVAL;
    if (!d->dconf && !d->dvalue) return USOT_OK;
    CfK p;
    cf_fill(d, lanes, p);
    hipLaunchKernelGGL(conf_fusion_bwd_f32, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int64_t usot_box_exp_ws_floats(const usot_box_exp_desc *d)
{
    if (!bx_geometry_ok(d)) return USOT_EINVAL;
    return (int64_t)BX_SUMS * bx_parts(d);
}

extern "C" int usot_box_exp_fwd_f32(void *stream, const usot_box_exp_desc *d)
{
    if (!bx_geometry_ok(d) || !d->p || !d->adjust || !d->bias || !d->y) return USOT_EINVAL;
    if (misaligned({d->p, d->adjust, d->bias, d->y})) return USOT_EINVAL;
    BxK p;
    bx_fill(d, p);
    hipLaunchKernelGGL(box_exp_fwd_f32, dim3((unsigned)p.parts), dim3(256), 0, (hipStream_t)stream, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_box_exp_bwd_f32(void *stream, const usot_box_exp_desc *d)
{
    if (!bx_geometry_ok(d) || !d->p || !d->adjust || !d->bias || !d->dy) return USOT_EINVAL;
    const bool sums = d->dadjust || d->dbias;
    if (sums && !d->ws) return USOT_EINVAL;
    if (misaligned({d->p, d->adjust, d->bias, d->dy, d->dp, d->dadjust, d->dbias, d->ws})) return USOT_EINVAL;
    if (!sums && !d->dp) return USOT_OK;
    BxK p;
    bx_fill(d, p);
    if (!sums) p.ws = nullptr;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(box_exp_bwd_f32, dim3((unsigned)p.parts), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    if (sums) {
        hipLaunchKernelGGL(box_exp_merge_f32, dim3(1), dim3(256), 0, s, p);
        USOT_CHECK_LAUNCH();
    }
    return USOT_OK;
}
