// BatchNorm2d on NHWC fp32 maps seen as [M][C] (M = N*H*W rows, C % 4 == 0), forward and gradients; usot_bn_desc in usot_hip.h
// states the arithmetic.  Everything here is bandwidth: a per-channel reduction over the rows, then an elementwise pass.
//
// Thread layout of all four kernels: 256 threads own a block of CB = 64 channels; thread t holds the four channels 4*(t & 15) ..
// + 3 (one float4: a row of the block is 256 contiguous bytes over 16 lanes) of the rows r with r % 16 == t >> 4.  A step is
// R = 64 rows: four independent 16-byte loads per thread and operand.
//
// (1) bn_stats_f32 / bn_bwd_sums_f32, grid (slices, channel blocks): a workgroup walks the steps of its slice.  A thread folds
//     the (up to) four rows of a step into (count, mean, M2) of their own - mean first, then squared distances to it - and merges
//     that into its running triple with Chan's formula; E[x^2] - E[x]^2 never appears.  The backward sums (dy', dy' * xhat) are
//     plain float sums built the same way (step sum, then running total).  The 16 row groups meet in LDS and thread c < 64 merges
//     them in row-group order (float64 from here on) and stores its channel's partial into ws[slice][2][C].  A slice without a
//     step returns at once.
// (2) bn_fwd_apply_f32 / bn_bwd_apply_f32, grid (row blocks, channel blocks): the prologue merges the slices' partials of the
//     workgroup's 64 channels - wavefront q takes slices q, q + 4, ... ascending, then thread c < 64 merges the four in order; the
//     counts come from the geometry, and a slice that owns no row is skipped without a load - and leaves per-channel
//     coefficients in LDS.  Every workgroup of a channel block computes the same bits; row block 0 alone stores save_mean,
//     save_invstd, the running statistics, dgamma and dbeta.  Then a grid-stride loop over the steps.
// The ReLU mask of the backward pass is recomputed: bn_pre() is the one place `pre` is formed, contraction is off inside it, and
// mean / invstd reach the backward pass as the very floats the forward used (save_*, or inv_std() of the running variance).
//
// The residual form (usot_bn_add_desc: y = act(pre + res), a bottleneck's bn3 - add - ReLU) is the RES = true instantiation of
// (2) and of bn_bwd_sums_f32: one more 16-byte load per row next to x, s = pre + res formed in bn_pre_add() alone, dres = dy'
// stored next to dx.  The statistics do not see the residual (bn_stats_f32 as it is).  RES = false takes the BnK argument block
// and compiles every residual line away: the plain entry points keep their instruction streams.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <initializer_list>
#include "usot_hip.h"
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CB = 64;                 // channels per workgroup
constexpr int RG = 16;                 // row groups of a workgroup (256 threads / 16 lanes per row)
constexpr int RPT = 4;                 // rows per thread and step
constexpr int R = RG * RPT;            // rows per step
constexpr int MAX_AUTO_SLICES = 64;

struct BnK {
    const float *x, *gamma, *beta, *mean, *var_or_invstd, *dy;
    float *rmean, *rvar, *y, *save_mean, *save_invstd, *dx, *dgamma, *dbeta, *ws;
    int M, C, steps, slices, training, act, reduce;
    float eps, momentum;
};

// the argument block of the residual instantiations: BnK as it is, then the residual and its gradient
struct BnAddK : BnK {
    const float *res;
    float *dres;
};
template <bool RES> struct Args { typedef BnK type; };
template <> struct Args<true> { typedef BnAddK type; };

__device__ __forceinline__ float inv_std(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// xhat and the pre-activation: the same three roundings wherever it is called
__device__ __forceinline__ float bn_pre(float x, float mean, float invstd, float g, float b, float &xhat)
{
#pragma clang fp contract(off)
    const float c = x - mean;
    xhat = c * invstd;
    return fmaf(xhat, g, b);
}

// the pre-activation of the residual form, s = pre + res: one float32 add behind bn_pre's three roundings, never contracted
__device__ __forceinline__ float bn_pre_add(float x, float mean, float invstd, float g, float b, float res, float &xhat)
{
#pragma clang fp contract(off)
    const float pre = bn_pre(x, mean, invstd, g, b, xhat);
    return pre + res;
}

__device__ __forceinline__ int slice_begin(int steps, int slices, int s) { return (int)((long)steps * s / slices); }

// rows of slice s: whole steps, the last one cut at M
__device__ __forceinline__ int slice_rows(int M, int steps, int slices, int s)
{
    const int s0 = slice_begin(steps, slices, s), s1 = slice_begin(steps, slices, s + 1);
    if (s1 <= s0) return 0;
    const long e = (long)s1 * R;
    return (int)((e < M ? e : (long)M) - (long)s0 * R);
}

// (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb), nb > 0
__device__ __forceinline__ void chan(float &na, float &ma, float &qa, float nb, float mb, float qb)
{
    const float n = na + nb, f = nb / n, dl = mb - ma;
    ma += dl * f;
    qa += qb + dl * dl * (na * f);
    na = n;
}

// the same merge in float64: row groups, slices and wavefronts meet through it (a few merges per thread, nothing per element), so
// the rounding of those stages - each would otherwise move the mean by up to half an ulp of its magnitude, not of the spread -
// stays out of the result
__device__ __forceinline__ void chan(double &na, double &ma, double &qa, double nb, double mb, double qb)
{
    const double n = na + nb, f = nb / n, dl = mb - ma;
    ma += dl * f;
    qa += qb + dl * dl * (na * f);
    na = n;
}

// rows of step `st` that belong to row group rg: row = st*R + j*RG + rg, j < k
__device__ __forceinline__ int rows_of(int M, int st, int rg)
{
    const long left = (long)M - (long)st * R - rg;
    if (left <= 0) return 0;
    const long k = (left + RG - 1) / RG;
    return k > RPT ? RPT : (int)k;
}

__global__ __launch_bounds__(256) void bn_stats_f32(const BnK p)
{
    __shared__ float sm[RG][2][CB];
    __shared__ float smn[RG];
    const int t = threadIdx.x, cl = t & 15, rg = t >> 4;
    const int s = blockIdx.x, c0 = blockIdx.y * CB;
    const int s0 = slice_begin(p.steps, p.slices, s), s1 = slice_begin(p.steps, p.slices, s + 1);
    if (s1 <= s0) return;
    const int c = c0 + 4 * cl;
    const bool live = c < p.C;
    float n = 0.f;
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    for (int st = s0; st < s1; ++st) {
        const int k = rows_of(p.M, st, rg);
        if (k == 0 || !live) continue;
        const float *xp = p.x + ((long)st * R + rg) * p.C + c;
        f32x4 v[RPT];
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) v[j] = *(const f32x4 *)(xp + (long)j * RG * p.C);
        f32x4 sum = v[0];
#pragma unroll
        for (int j = 1; j < RPT; ++j)
            if (j < k) sum += v[j];
        const float nb = (float)k;
        const f32x4 mb = sum / nb;
        f32x4 qb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) {
                const f32x4 dv = v[j] - mb;
                qb += dv * dv;
            }
        const float nn = n + nb, f = nb / nn;
        const f32x4 dl = mb - mean;
        mean += dl * f;
        m2 += qb + dl * dl * (n * f);
        n = nn;
    }
    *(f32x4 *)&sm[rg][0][4 * cl] = mean;
    *(f32x4 *)&sm[rg][1][4 * cl] = m2;
    if (cl == 0) smn[rg] = live ? n : 0.f;
    __syncthreads();
    if (t < CB && c0 + t < p.C) {
        double na = 0., ma = 0., qa = 0.;
        for (int g = 0; g < RG; ++g) {
            const float nb = smn[g];
            if (nb > 0.f) chan(na, ma, qa, (double)nb, (double)sm[g][0][t], (double)sm[g][1][t]);
        }
        float *w = p.ws + (long)s * 2 * p.C + c0 + t;
        w[0] = (float)ma;
        w[p.C] = (float)qa;
    }
}

template <bool RES>
__global__ __launch_bounds__(256) void bn_fwd_apply_f32(const typename Args<RES>::type p)
{
    __shared__ double sm[4][2][CB];
    __shared__ double smn[4];
    __shared__ __attribute__((aligned(16))) float co[4][CB];      // mean, invstd, gamma, beta
    const int t = threadIdx.x, c0 = blockIdx.y * CB;
    if (p.training) {
        const int cc = t & 63, q = t >> 6;
        double na = 0., ma = 0., qa = 0.;
        if (c0 + cc < p.C)
            for (int s = q; s < p.slices; s += 4) {
                const int rows = slice_rows(p.M, p.steps, p.slices, s);
                if (rows == 0) continue;
                const float *w = p.ws + (long)s * 2 * p.C + c0 + cc;
                chan(na, ma, qa, (double)rows, (double)w[0], (double)w[p.C]);
            }
        sm[q][0][cc] = ma;
        sm[q][1][cc] = qa;
        if (cc == 0) smn[q] = na;       // channel c0 always exists
        __syncthreads();
    }
    if (t < CB) {
        const int c = c0 + t;
        float mean = 0.f, is = 0.f, g = 0.f, b = 0.f;
        if (c < p.C) {
            g = p.gamma[c];
            b = p.beta[c];
            if (p.training) {
                double na = 0., ma = 0., qa = 0.;
                for (int q = 0; q < 4; ++q)
                    if (smn[q] > 0.) chan(na, ma, qa, smn[q], sm[q][0][t], sm[q][1][t]);
                mean = (float)ma;
                is = (float)(1.0 / sqrt(qa / (double)p.M + (double)p.eps));
                if (blockIdx.x == 0) {
                    p.save_mean[c] = mean;
                    p.save_invstd[c] = is;
                    if (p.rmean) p.rmean[c] = (1.f - p.momentum) * p.rmean[c] + p.momentum * mean;
                    if (p.rvar) p.rvar[c] = (1.f - p.momentum) * p.rvar[c] + p.momentum * (float)(qa / (double)(p.M - 1));
                }
            } else {
                mean = p.mean[c];
                is = inv_std(p.var_or_invstd[c], p.eps);
            }
        }
        co[0][t] = mean; co[1][t] = is; co[2][t] = g; co[3][t] = b;
    }
    __syncthreads();
    const int cl = t & 15, rg = t >> 4, c = c0 + 4 * cl;
    if (c >= p.C) return;
    const f32x4 mean = *(const f32x4 *)&co[0][4 * cl], is = *(const f32x4 *)&co[1][4 * cl];
    const f32x4 g = *(const f32x4 *)&co[2][4 * cl], b = *(const f32x4 *)&co[3][4 * cl];
    for (int st = blockIdx.x; st < p.steps; st += gridDim.x) {
        const int k = rows_of(p.M, st, rg);
        const long off = ((long)st * R + rg) * p.C + c;
        f32x4 v[RPT], r[RPT];
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) {
                v[j] = *(const f32x4 *)(p.x + off + (long)j * RG * p.C);
                if constexpr (RES) r[j] = *(const f32x4 *)(p.res + off + (long)j * RG * p.C);
            }
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xh, pre;
                    if constexpr (RES) pre = bn_pre_add(v[j][e], mean[e], is[e], g[e], b[e], r[j][e], xh);
                    else pre = bn_pre(v[j][e], mean[e], is[e], g[e], b[e], xh);
                    o[e] = p.act ? (pre > 0.f ? pre : 0.f) : pre;
                }
                *(f32x4 *)(p.y + off + (long)j * RG * p.C) = o;
            }
    }
}

// mean / invstd of the four channels of a thread, as the forward used them
__device__ __forceinline__ void load_stats(const BnK &p, int c, f32x4 &mean, f32x4 &is)
{
    mean = *(const f32x4 *)(p.mean + c);
    const f32x4 v = *(const f32x4 *)(p.var_or_invstd + c);
    if (p.training) is = v;
    else
#pragma unroll
        for (int e = 0; e < 4; ++e) is[e] = inv_std(v[e], p.eps);
}

template <bool RES>
__global__ __launch_bounds__(256) void bn_bwd_sums_f32(const typename Args<RES>::type p)
{
    __shared__ float sm[RG][2][CB];
    const int t = threadIdx.x, cl = t & 15, rg = t >> 4;
    const int s = blockIdx.x, c0 = blockIdx.y * CB;
    const int s0 = slice_begin(p.steps, p.slices, s), s1 = slice_begin(p.steps, p.slices, s + 1);
    if (s1 <= s0) return;
    const int c = c0 + 4 * cl;
    f32x4 sb = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
    if (c < p.C) {
        f32x4 mean, is, g = *(const f32x4 *)(p.gamma + c), b = {0.f, 0.f, 0.f, 0.f};
        load_stats(p, c, mean, is);
        if (p.act) b = *(const f32x4 *)(p.beta + c);
        for (int st = s0; st < s1; ++st) {
            const int k = rows_of(p.M, st, rg);
            const long off = ((long)st * R + rg) * p.C + c;
            f32x4 v[RPT], d[RPT], r[RPT];
#pragma unroll
            for (int j = 0; j < RPT; ++j)
                if (j < k) {
                    v[j] = *(const f32x4 *)(p.x + off + (long)j * RG * p.C);
                    d[j] = *(const f32x4 *)(p.dy + off + (long)j * RG * p.C);
                    if constexpr (RES) r[j] = p.act ? *(const f32x4 *)(p.res + off + (long)j * RG * p.C) : d[j];   // the mask alone reads it
                }
            f32x4 tb = {0.f, 0.f, 0.f, 0.f}, tg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < RPT; ++j)
                if (j < k) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float xh, pre;
                        if constexpr (RES) pre = bn_pre_add(v[j][e], mean[e], is[e], g[e], b[e], r[j][e], xh);
                        else pre = bn_pre(v[j][e], mean[e], is[e], g[e], b[e], xh);
                        const float dd = (p.act && !(pre > 0.f)) ? 0.f : d[j][e];
                        tb[e] += dd;
                        tg[e] = fmaf(dd, xh, tg[e]);
                    }
                }
            sb += tb;
            sg += tg;
        }
    }
    *(f32x4 *)&sm[rg][0][4 * cl] = sb;
    *(f32x4 *)&sm[rg][1][4 * cl] = sg;
    __syncthreads();
    if (t < CB && c0 + t < p.C) {
        float a = 0.f, b = 0.f;
        for (int g = 0; g < RG; ++g) {
            a += sm[g][0][t];
            b += sm[g][1][t];
        }
        float *w = p.ws + (long)s * 2 * p.C + c0 + t;
        w[0] = a;
        w[p.C] = b;
    }
}

template <bool RES>
__global__ __launch_bounds__(256) void bn_bwd_apply_f32(const typename Args<RES>::type p)
{
    __shared__ float sm[4][2][CB];
    __shared__ __attribute__((aligned(16))) float co[2][CB];      // dbeta / M, dgamma / M
    const int t = threadIdx.x, c0 = blockIdx.y * CB;
    if (p.reduce) {
        const int cc = t & 63, q = t >> 6;
        float a = 0.f, b = 0.f;
        if (c0 + cc < p.C)
            for (int s = q; s < p.slices; s += 4) {
                if (slice_rows(p.M, p.steps, p.slices, s) == 0) continue;
                const float *w = p.ws + (long)s * 2 * p.C + c0 + cc;
                a += w[0];
                b += w[p.C];
            }
        sm[q][0][cc] = a;
        sm[q][1][cc] = b;
        __syncthreads();
        if (t < CB) {
            float db = 0.f, dg = 0.f;
            for (int qq = 0; qq < 4; ++qq) {
                db += sm[qq][0][t];
                dg += sm[qq][1][t];
            }
            if (blockIdx.x == 0 && c0 + t < p.C) {
                if (p.dbeta) p.dbeta[c0 + t] = db;
                if (p.dgamma) p.dgamma[c0 + t] = dg;
            }
            co[0][t] = db / (float)p.M;
            co[1][t] = dg / (float)p.M;
        }
        __syncthreads();
    }
    if constexpr (RES) {
        if (!p.dx && !p.dres) return;
    } else {
        if (!p.dx) return;
    }
    const int cl = t & 15, rg = t >> 4, c = c0 + 4 * cl;
    if (c >= p.C) return;
    f32x4 mean, is, kb = {0.f, 0.f, 0.f, 0.f}, kg = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    const f32x4 g = *(const f32x4 *)(p.gamma + c);
    load_stats(p, c, mean, is);
    if (p.act) b = *(const f32x4 *)(p.beta + c);
    bool coeffs = p.training;
    if constexpr (RES) coeffs = p.training && p.dx;      // dres alone: no reduction ran, and x is read for the mask only
    if (coeffs) {
        kb = *(const f32x4 *)&co[0][4 * cl];
        kg = *(const f32x4 *)&co[1][4 * cl];
    }
    const f32x4 a = g * is;
    const bool need_x = p.act || coeffs;
    for (int st = blockIdx.x; st < p.steps; st += gridDim.x) {
        const int k = rows_of(p.M, st, rg);
        const long off = ((long)st * R + rg) * p.C + c;
        f32x4 v[RPT], d[RPT], r[RPT];
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) {
                d[j] = *(const f32x4 *)(p.dy + off + (long)j * RG * p.C);
                v[j] = need_x ? *(const f32x4 *)(p.x + off + (long)j * RG * p.C) : d[j];
                if constexpr (RES) r[j] = p.act ? *(const f32x4 *)(p.res + off + (long)j * RG * p.C) : d[j];
            }
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (j < k) {
                f32x4 o;
                [[maybe_unused]] f32x4 m;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xh, pre;
                    if constexpr (RES) pre = bn_pre_add(v[j][e], mean[e], is[e], g[e], b[e], r[j][e], xh);
                    else pre = bn_pre(v[j][e], mean[e], is[e], g[e], b[e], xh);
                    const float dd = (p.act && !(pre > 0.f)) ? 0.f : d[j][e];
                    o[e] = p.training ? a[e] * (dd - kb[e] - xh * kg[e]) : a[e] * dd;
                    if constexpr (RES) m[e] = dd;
                }
                if constexpr (RES) {
                    if (p.dx) *(f32x4 *)(p.dx + off + (long)j * RG * p.C) = o;
                    if (p.dres) *(f32x4 *)(p.dres + off + (long)j * RG * p.C) = m;
                } else {
                    *(f32x4 *)(p.dx + off + (long)j * RG * p.C) = o;
                }
            }
    }
}

int device_cus()
{
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        return prop.multiProcessorCount;
    return 256;
}

int bn_geometry_ok(const usot_bn_desc *d)
{
    if (!d) return 0;
    if (d->C < 4 || (d->C & 3) || d->C > 65535 * CB) return 0;     // channel blocks are the grid's y
    if (d->training != 0 && d->training != 1) return 0;
    if (d->act != USOT_ACT_NONE && d->act != USOT_ACT_RELU) return 0;
    if (d->M < (d->training ? 2 : 1)) return 0;
    if (d->slices < 0 || d->slices > d->M) return 0;
    if (!(d->eps >= 0.f) || !isfinite(d->eps) || !isfinite(d->momentum)) return 0;
    return 1;
}

int steps_of(const usot_bn_desc *d) { return (int)(((long)d->M + R - 1) / R); }
int cblocks_of(const usot_bn_desc *d) { return (d->C + CB - 1) / CB; }

// about two workgroups per compute unit, no slice below two steps, at most MAX_AUTO_SLICES (the second launch's prologue walks them)
int auto_slices(const usot_bn_desc *d)
{
    long s = (2L * device_cus() + cblocks_of(d) - 1) / cblocks_of(d);
    const long most = steps_of(d) / 2;
    if (s > most) s = most;
    if (s > MAX_AUTO_SLICES) s = MAX_AUTO_SLICES;
    return s < 1 ? 1 : (int)s;
}

bool misaligned(std::initializer_list<const void *> ps)
{
    uintptr_t a = 0;
    for (const void *q : ps) a |= (uintptr_t)q;
    return (a & 15) != 0;
}

void fill(const usot_bn_desc *d, BnK &p);
void fill(const usot_bn_add_desc *d, BnAddK &p)
{
    fill(&d->bn, p);
    p.res = d->res; p.dres = d->dres;
}

void fill(const usot_bn_desc *d, BnK &p)
{
    p.x = d->x; p.gamma = d->gamma; p.beta = d->beta; p.dy = d->dy;
    p.mean = d->training ? d->save_mean : d->running_mean;
    p.var_or_invstd = d->training ? d->save_invstd : d->running_var;
    p.rmean = d->running_mean; p.rvar = d->running_var;
    p.y = d->y; p.save_mean = d->save_mean; p.save_invstd = d->save_invstd;
    p.dx = d->dx; p.dgamma = d->dgamma; p.dbeta = d->dbeta; p.ws = d->ws;
    p.M = d->M; p.C = d->C; p.steps = steps_of(d);
    p.slices = d->slices > 0 ? d->slices : auto_slices(d);
    p.training = d->training; p.act = d->act; p.reduce = 0;
    p.eps = d->eps; p.momentum = d->momentum;
}

// row blocks of the elementwise launches: every step its own workgroup up to about eight workgroups per compute unit
unsigned apply_blocks(const BnK &p, int cblocks)
{
    long most = 8L * device_cus() / cblocks;
    if (most < 1) most = 1;
    return (unsigned)(p.steps < most ? p.steps : most);
}

}  // namespace

extern "C" int usot_batchnorm_geometry(int *rows, int *chans)
{
    if (rows) *rows = R;
    if (chans) *chans = CB;
    return USOT_OK;
}

extern "C" int usot_batchnorm_slices(const usot_bn_desc *d)
{
    if (!bn_geometry_ok(d)) return USOT_EINVAL;
    return d->slices > 0 ? d->slices : auto_slices(d);
}

extern "C" int64_t usot_batchnorm_ws_floats(const usot_bn_desc *d)
{
    const int s = usot_batchnorm_slices(d);
    if (s < 0) return s;
    return (int64_t)2 * s * d->C;
}

extern "C" int usot_batchnorm_fwd_f32(void *stream, const usot_bn_desc *d)
{
    if (!bn_geometry_ok(d) || !d->x || !d->gamma || !d->beta || !d->y) return USOT_EINVAL;
    if (d->training ? (!d->save_mean || !d->save_invstd || !d->ws) : (!d->running_mean || !d->running_var)) return USOT_EINVAL;
    if (misaligned({d->x, d->gamma, d->beta, d->y, d->running_mean, d->running_var})) return USOT_EINVAL;
    if (d->training && misaligned({d->save_mean, d->save_invstd, d->ws})) return USOT_EINVAL;
    BnK p;
    fill(d, p);
    const int cb = cblocks_of(d);
    hipStream_t s = (hipStream_t)stream;
    if (d->training) {
        hipLaunchKernelGGL(bn_stats_f32, dim3((unsigned)p.slices, (unsigned)cb), dim3(256), 0, s, p);
        USOT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bn_fwd_apply_f32<false>, dim3(apply_blocks(p, cb), (unsigned)cb), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_batchnorm_bwd_f32(void *stream, const usot_bn_desc *d)
{
    if (!bn_geometry_ok(d) || !d->x || !d->gamma || !d->dy || (d->act && !d->beta)) return USOT_EINVAL;
    if (d->training ? (!d->save_mean || !d->save_invstd) : (!d->running_mean || !d->running_var)) return USOT_EINVAL;
    const bool sums = d->dgamma || d->dbeta || (d->training && d->dx);
    if (sums && !d->ws) return USOT_EINVAL;
    if (misaligned({d->x, d->gamma, d->beta, d->dy, d->dx, d->dgamma, d->dbeta, d->ws})) return USOT_EINVAL;
    if (d->training ? misaligned({d->save_mean, d->save_invstd}) : misaligned({d->running_mean, d->running_var})) return USOT_EINVAL;
    if (!sums && !d->dx) return USOT_OK;
    BnK p;
    fill(d, p);
    p.reduce = sums ? 1 : 0;
    const int cb = cblocks_of(d);
    hipStream_t s = (hipStream_t)stream;
    if (sums) {
        hipLaunchKernelGGL(bn_bwd_sums_f32<false>, dim3((unsigned)p.slices, (unsigned)cb), dim3(256), 0, s, p);
        USOT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bn_bwd_apply_f32<false>, dim3(d->dx ? apply_blocks(p, cb) : 1u, (unsigned)cb), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_batchnorm_add_fwd_f32(void *stream, const usot_bn_add_desc *a)
{
    if (!a) return USOT_EINVAL;
    const usot_bn_desc *d = &a->bn;
    if (!bn_geometry_ok(d) || !d->x || !d->gamma || !d->beta || !d->y || !a->res) return USOT_EINVAL;
    if (d->training ? (!d->save_mean || !d->save_invstd || !d->ws) : (!d->running_mean || !d->running_var)) return USOT_EINVAL;
    if (misaligned({d->x, d->gamma, d->beta, d->y, d->running_mean, d->running_var, a->res, a->dres})) return USOT_EINVAL;
    if (d->training && misaligned({d->save_mean, d->save_invstd, d->ws})) return USOT_EINVAL;
    BnAddK p;
    fill(a, p);
    const int cb = cblocks_of(d);
    hipStream_t s = (hipStream_t)stream;
    if (d->training) {
        hipLaunchKernelGGL(bn_stats_f32, dim3((unsigned)p.slices, (unsigned)cb), dim3(256), 0, s, (const BnK &)p);
        USOT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bn_fwd_apply_f32<true>, dim3(apply_blocks(p, cb), (unsigned)cb), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_batchnorm_add_bwd_f32(void *stream, const usot_bn_add_desc *a)
{
    if (!a) return USOT_EINVAL;
    const usot_bn_desc *d = &a->bn;
    if (!bn_geometry_ok(d) || !d->x || !d->gamma || !d->dy || !a->res || (d->act && !d->beta)) return USOT_EINVAL;
    if (d->training ? (!d->save_mean || !d->save_invstd) : (!d->running_mean || !d->running_var)) return USOT_EINVAL;
    if (!d->dx && !d->dgamma && !d->dbeta && !a->dres) return USOT_EINVAL;
    const bool sums = d->dgamma || d->dbeta || (d->training && d->dx);
    if (sums && !d->ws) return USOT_EINVAL;
    if (misaligned({d->x, d->gamma, d->beta, d->dy, d->dx, d->dgamma, d->dbeta, d->ws, a->res, a->dres})) return USOT_EINVAL;
    if (d->training ? misaligned({d->save_mean, d->save_invstd}) : misaligned({d->running_mean, d->running_var})) return USOT_EINVAL;
    BnAddK p;
    fill(a, p);
    p.reduce = sums ? 1 : 0;
    const int cb = cblocks_of(d);
    hipStream_t s = (hipStream_t)stream;
    if (sums) {
        hipLaunchKernelGGL(bn_bwd_sums_f32<true>, dim3((unsigned)p.slices, (unsigned)cb), dim3(256), 0, s, p);
        USOT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bn_bwd_apply_f32<true>, dim3(d->dx || a->dres ? apply_blocks(p, cb) : 1u, (unsigned)cb), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}
