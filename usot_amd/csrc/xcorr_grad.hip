// Gradients of the depthwise cross-correlation on NCHW planes (reference lib/models/connect.py:147-157;
// forward: xcorr_planes_kernel in xcorr.hip).  For P planes, x [P][Hx][Wx], k [P][Hk][Wk], dout [P][OH][OW]:
//
//   dx[p][a][b] = scale * sum_{u,v} dout[p][a-u][b-v] * k[p][u][v]          (terms outside dout are 0)
//   dk[p][u][v] = scale * sum_{i,j} dout[p][i][j]     * x[p][i+u][j+v]
//
// Like the forward these are 25 MACs per element against ~7 bytes of compulsory traffic: streaming work, not a dense
// contraction, so neither touches MFMA (measured rates and what limits them: DESIGN.md 3.3.1).  Every output element
// is written once, by one thread, with a plain store: no atomics, no memset, no workspace, and the order of every
// sum is fixed by the code, so equal inputs give equal bits.
//
// (1) xcorr_bwd_x_kernel: the forward's rolling-window kernel run "full".  One wavefront per plane (two when
//     Wx <= 32); lane b owns column b of dx, keeps the HK most recent rows of dout (zero rows above and below the
//     map) at columns b .. b-WK+1, the shifted columns coming from the lower neighbours by wavefront shuffles,
//     once per dout row; the template sits in LDS and is read into registers by broadcast.
// (2) xcorr_bwd_k_kernel: a reduction.  Lane j owns column j of dout, walks the rows once with the HK most
//     recent rows of x at columns j .. j+WK-1 in registers (loads one row ahead) and keeps HK*WK partial sums (one per tap); an xor
//     butterfly over the wavefront (its half with two planes per wavefront) finishes them and lanes 0 .. HK*WK-1
//     store one tap each.  Order of summation: rows ascending inside a lane, then the butterfly's fixed tree.
// (3) generic kernels, one thread per output element, for every other template size and Wx > 64 (correctness only).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "usot_hip.h"
#include "common.h"

namespace {

template <int HK, int WK>
__global__ __launch_bounds__(256) void xcorr_bwd_x_kernel(
    const float *__restrict__ dout, const float *__restrict__ k, float *__restrict__ dx,
    int P, int Hx, int Wx, int per_wave, float scale)
{
    __shared__ float tz[4][2][HK * WK];          // template tiles of this block's waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int OHh = Hx - HK + 1, OWw = Wx - WK + 1;
    const int half = per_wave == 2 ? (lane >> 5) : 0;
    const int j = per_wave == 2 ? (lane & 31) : lane;
    const int nunits = (P + per_wave - 1) / per_wave;
    for (int unit = blockIdx.x * 4 + wave; unit < nunits; unit += gridDim.x * 4) {
        const int plane = unit * per_wave + half;
        const bool live = plane < P;
        for (int t = lane; t < per_wave * HK * WK; t += 64) {
            const int h = t / (HK * WK), e = t - h * HK * WK;
            const int pl = unit * per_wave + h;
            tz[wave][h][e] = pl < P ? k[(long)pl * HK * WK + e] : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
        float kt[HK][WK];
#pragma unroll
        for (int u = 0; u < HK; ++u)
#pragma unroll
            for (int v = 0; v < WK; ++v) kt[u][v] = tz[wave][half][u * WK + v];

        const float *dp = dout + (long)(live ? plane : 0) * OHh * OWw;
        float *xp = dx + (long)(live ? plane : 0) * Hx * Wx;
        // win[t][v] = dout[row a-(HK-1)+t][j-v]; the shifted copies come from lane j-v (zero left of the map:
        // a lane below v would otherwise see its own value or, with two planes per wavefront, the other plane's)
        float win[HK][WK];
#pragma unroll
        for (int t = 0; t < HK; ++t)
#pragma unroll
            for (int v = 0; v < WK; ++v) win[t][v] = 0.f;
        for (int a = 0; a < Hx; ++a) {
#pragma unroll
            for (int t = 0; t < HK - 1; ++t)
#pragma unroll
                for (int v = 0; v < WK; ++v) win[t][v] = win[t + 1][v];
            const float dv = (live && a < OHh && j < OWw) ? dp[(long)a * OWw + j] : 0.f;
            win[HK - 1][0] = dv;
#pragma unroll
            for (int v = 1; v < WK; ++v) {
                const float s = __shfl_up(dv, v, 64);
                win[HK - 1][v] = j >= v ? s : 0.f;
            }
            // dx[a][j] = sum_u sum_v dout[a-u][j-v] k[u][v], dout[a-u] = win[HK-1-u]
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < HK; ++u)
#pragma unroll
                for (int v = 0; v < WK; ++v) acc = fmaf(win[HK - 1 - u][v], kt[u][v], acc);
            if (live && j < Wx) xp[(long)a * Wx + j] = acc * scale;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int HK, int WK>
__global__ __launch_bounds__(256) void xcorr_bwd_k_kernel(
    const float *__restrict__ dout, const float *__restrict__ x, float *__restrict__ dk,
    int P, int Hx, int Wx, int per_wave, float scale)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int OHh = Hx - HK + 1, OWw = Wx - WK + 1;
    const int half = per_wave == 2 ? (lane >> 5) : 0;
    const int j = per_wave == 2 ? (lane & 31) : lane;
    const int nunits = (P + per_wave - 1) / per_wave;
    for (int unit = blockIdx.x * 4 + wave; unit < nunits; unit += gridDim.x * 4) {
        const int plane = unit * per_wave + half;
        const bool live = plane < P;
        const float *dp = dout + (long)(live ? plane : 0) * OHh * OWw;
        const float *xp = x + (long)(live ? plane : 0) * Hx * Wx;
        // win[u][v] = x[row r-(HK-1)+u][j+v], zero in the lanes right of dout's last column (their dout is zero
        // too; the mask keeps another plane's or a stale lane's inf / NaN out of 0 * x)
        float win[HK][WK], acc[HK][WK];
#pragma unroll
        for (int u = 0; u < HK; ++u)
#pragma unroll
            for (int v = 0; v < WK; ++v) win[u][v] = acc[u][v] = 0.f;
        const bool col = j < OWw;
        // both loads run one row ahead of their use (rows 0 of x and of dout first): the kernel waits on two loads per
        // row, and one row of lookahead is worth 8 - 30 % of its time; bwd_x, one load per row, gains nothing
        float xn = (live && j < Wx) ? xp[j] : 0.f;
        float dn = (live && col && HK == 1) ? dp[j] : 0.f;
        for (int r = 0; r < Hx; ++r) {
#pragma unroll
            for (int u = 0; u < HK - 1; ++u)
#pragma unroll
                for (int v = 0; v < WK; ++v) win[u][v] = win[u + 1][v];
            const float xv = xn, d = dn;
            const int i = r - (HK - 1);
            if (r + 1 < Hx) {
                xn = (live && j < Wx) ? xp[(long)(r + 1) * Wx + j] : 0.f;
                dn = (live && col && i + 1 >= 0) ? dp[(long)(i + 1) * OWw + j] : 0.f;
            }
            win[HK - 1][0] = col ? xv : 0.f;
#pragma unroll
            for (int v = 1; v < WK; ++v) {
                const float s = __shfl_down(xv, v, 64);
                win[HK - 1][v] = col ? s : 0.f;
            }
            if (i >= 0) {
#pragma unroll
                for (int u = 0; u < HK; ++u)
#pragma unroll
                    for (int v = 0; v < WK; ++v) acc[u][v] = fmaf(d, win[u][v], acc[u][v]);
            }
        }
        // butterfly over the plane's lanes: every lane ends with all HK*WK sums, lane t keeps tap t
        float mine = 0.f;
#pragma unroll
        for (int u = 0; u < HK; ++u)
#pragma unroll
            for (int v = 0; v < WK; ++v) {
                float s = acc[u][v];
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                s += __shfl_xor(s, 8, 64);
                s += __shfl_xor(s, 16, 64);
                if (per_wave == 1) s += __shfl_xor(s, 32, 64);
                if (j == u * WK + v) mine = s;
            }
        if (live && j < HK * WK) dk[(long)plane * HK * WK + j] = mine * scale;
    }
}

// any template size: one thread per gradient element (slow path, correctness only)
__global__ __launch_bounds__(256) void xcorr_bwd_x_generic(
    const float *__restrict__ dout, const float *__restrict__ k, float *__restrict__ dx,
    int P, int Hx, int Wx, int Hk, int Wk, float scale)
{
    const int OHh = Hx - Hk + 1, OWw = Wx - Wk + 1;
    const long total = (long)P * Hx * Wx;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx % Wx);
        const int a = (int)((idx / Wx) % Hx);
        const long pl = idx / ((long)Wx * Hx);
        float acc = 0.f;
        for (int u = 0; u < Hk; ++u) {
            const int i = a - u;
            if (i < 0 || i >= OHh) continue;
            for (int v = 0; v < Wk; ++v) {
                const int jj = b - v;
                if (jj < 0 || jj >= OWw) continue;
                acc = fmaf(dout[(pl * OHh + i) * OWw + jj], k[(pl * Hk + u) * Wk + v], acc);
            }
        }
        dx[idx] = acc * scale;
    }
}

__global__ __launch_bounds__(256) void xcorr_bwd_k_generic(
    const float *__restrict__ dout, const float *__restrict__ x, float *__restrict__ dk,
    int P, int Hx, int Wx, int Hk, int Wk, float scale)
{
    const int OHh = Hx - Hk + 1, OWw = Wx - Wk + 1;
    const long total = (long)P * Hk * Wk;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int v = (int)(idx % Wk);
        const int u = (int)((idx / Wk) % Hk);
        const long pl = idx / ((long)Wk * Hk);
        float acc = 0.f;
        for (int i = 0; i < OHh; ++i) {
            float row = 0.f;                    // row sums first: shorter chains than one OH*OW-long accumulation
            for (int jj = 0; jj < OWw; ++jj)
                row = fmaf(dout[(pl * OHh + i) * OWw + jj], x[(pl * Hx + i + u) * Wx + jj + v], row);
            acc += row;
        }
        dk[idx] = acc * scale;
    }
}

int planes_blocks(int P, int per_wave)
{
    const int nunits = (P + per_wave - 1) / per_wave;
    const int blocks = (nunits + 3) / 4;
    return blocks > 4096 ? 4096 : blocks;
}

template <int HK, int WK>
int launch_bwd_x(hipStream_t s, const float *dout, const float *k, float *dx, int P, int Hx, int Wx, float scale)
{
    const int per_wave = Wx <= 32 ? 2 : 1;
    hipLaunchKernelGGL((xcorr_bwd_x_kernel<HK, WK>), dim3(planes_blocks(P, per_wave)), dim3(256), 0, s,
                       dout, k, dx, P, Hx, Wx, per_wave, scale);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

template <int HK, int WK>
int launch_bwd_k(hipStream_t s, const float *dout, const float *x, float *dk, int P, int Hx, int Wx, float scale)
{
    const int per_wave = Wx <= 32 ? 2 : 1;
    hipLaunchKernelGGL((xcorr_bwd_k_kernel<HK, WK>), dim3(planes_blocks(P, per_wave)), dim3(256), 0, s,
                       dout, x, dk, P, Hx, Wx, per_wave, scale);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

int generic_blocks(long total)
{
    const long b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : b);
}

}  // namespace

extern "C" int usot_xcorr_depthwise_bwd_x_f32(void *stream, const float *dout, const float *k, float *dx,
                                              int P, int Hx, int Wx, int Hk, int Wk, float scale)
{
    if (!dout || !k || !dx || P < 0 || Hk < 1 || Wk < 1 || Hx < Hk || Wx < Wk) return USOT_EINVAL;
    if (P == 0) return USOT_OK;
    hipStream_t s = (hipStream_t)stream;
    if (Wx <= 64) {
        if (Hk == 5 && Wk == 5) return launch_bwd_x<5, 5>(s, dout, k, dx, P, Hx, Wx, scale);
        if (Hk == 3 && Wk == 5) return launch_bwd_x<3, 5>(s, dout, k, dx, P, Hx, Wx, scale);
        if (Hk == 5 && Wk == 3) return launch_bwd_x<5, 3>(s, dout, k, dx, P, Hx, Wx, scale);
    }
    hipLaunchKernelGGL(xcorr_bwd_x_generic, dim3(generic_blocks((long)P * Hx * Wx)), dim3(256), 0, s,
                       dout, k, dx, P, Hx, Wx, Hk, Wk, scale);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_xcorr_depthwise_bwd_k_f32(void *stream, const float *dout, const float *x, float *dk,
                                              int P, int Hx, int Wx, int Hk, int Wk, float scale)
{
    if (!dout || !x || !dk || P < 0 || Hk < 1 || Wk < 1 || Hx < Hk || Wx < Wk) return USOT_EINVAL;
    if (P == 0) return USOT_OK;
    hipStream_t s = (hipStream_t)stream;
    if (Wx <= 64) {
        if (Hk == 5 && Wk == 5) return launch_bwd_k<5, 5>(s, dout, x, dk, P, Hx, Wx, scale);
        if (Hk == 3 && Wk == 5) return launch_bwd_k<3, 5>(s, dout, x, dk, P, Hx, Wx, scale);
        if (Hk == 5 && Wk == 3) return launch_bwd_k<5, 3>(s, dout, x, dk, P, Hx, Wx, scale);
    }
    hipLaunchKernelGGL(xcorr_bwd_k_generic, dim3(generic_blocks((long)P * Hk * Wk)), dim3(256), 0, s,
                       dout, x, dk, P, Hx, Wx, Hk, Wk, scale);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}
