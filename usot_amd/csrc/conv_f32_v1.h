// v1: conv_igemm_f32 - 256 threads = 4 wavefronts that load AND multiply, two LDS stages of 32 k, one barrier per k-tile (the
// scheme the comment at the head of conv_igemm.hip describes).  Routed for the batched backbone and the tiny-M encoders.
// DBG > 0 are timing forms (1: no global loads in the loop, 2: no fragment reads either); only DBG = 0 is instantiated.
#pragma once
#include "conv_f32_common.h"

namespace {

template <int BM, int BN>
struct V1Geom { static constexpr int threads = 256, lds_bytes = 2 * (BM + BN) * LDK * 4; };      // two stages of [BM | BN] rows
template <int BM, int BN, int WM, int WN, int DBG = 0>
__global__ __launch_bounds__((V1Geom<BM, BN>::threads)) void conv_igemm_f32(const ConvBatch bt)
{
    int pi = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (q < bt.n && (int)blockIdx.x >= bt.start[q]) pi = q;
    const ConvK &p = bt.p[pi];
    const int bid0 = (int)blockIdx.x - bt.start[pi];
    static_assert(WM * WN == 4, "4 wavefronts per workgroup");
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    static_assert(TM >= 1 && TN >= 1, "wave tile at least 16x16");
    constexpr int XI = (BM + 31) / 32, WI = (BN + 31) / 32;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sX = smem;                   // [2][BM][LDK]
    float *sW = smem + 2 * BM * LDK;    // [2][BN][LDK]

    const int tid = threadIdx.x;
    const int tiles = p.MT * p.NT;
    const int total = tiles * p.groups * p.ksplit;
    const int b = xcd_remap(bid0, total);
    const int z = b / tiles, t = b - z * tiles;
    const int g = z / p.ksplit, ks = z - g * p.ksplit;
    const int bn0 = (t / p.MT) * BN, bm0 = (t % p.MT) * BM;
    const int kt0 = (int)((long)p.KT * ks / p.ksplit);
    const int kt1 = (int)((long)p.KT * (ks + 1) / p.ksplit);

    const float *__restrict__ xg = p.x + (long)g * p.x_gs;
    const float *__restrict__ wg = p.w + (long)g * p.w_gs;

    // ---- loader role: thread (lr, kc) moves 16-byte chunk kc of rows lr, lr+32, ...
    const int lr = tid >> 3, kc = tid & 7;
    int x_ih0[XI], x_iw0[XI];
    long x_nb[XI];
    bool x_ok[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int row = lr + 32 * i;
        const int m = bm0 + row;
        x_ok[i] = (row < BM) && (m < p.M);
        const int mm = x_ok[i] ? m : 0;
        const int n = mm / p.P, pix = mm - n * p.P;
        const int oh = pix / p.OW, ow = pix - oh * p.OW;
        x_ih0[i] = oh * p.stride - p.pad_h;
        x_iw0[i] = ow * p.stride - p.pad_w;
        x_nb[i] = (long)n * p.H * p.W * p.Cin + kc * 4;
    }
    long w_off[WI];
    bool w_ok[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = lr + 32 * i;
        const int co = bn0 + row;
        w_ok[i] = (row < BN) && (co < p.Cout);
        w_off[i] = (long)(w_ok[i] ? co : 0) * p.K + kc * 4;
    }

    f32x4 xr[XI], wr[WI];
    auto load_tile = [&](int kt) {
        const int tap = kt / p.cchunks, c0 = (kt - tap * p.cchunks) * 32;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        const int dh = kh * p.dil_h, dw = kw * p.dil_w;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int ih = x_ih0[i] + dh, iw = x_iw0[i] + dw;
            const bool ok = x_ok[i] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *(const f32x4 *)(xg + x_nb[i] + ((long)ih * p.W + iw) * p.Cin + c0);
            xr[i] = v;
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (w_ok[i]) v = *(const f32x4 *)(wg + w_off[i] + (long)kt * 32);
            wr[i] = v;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < XI; ++i)
            if (lr + 32 * i < BM)
                *(f32x4 *)(sX + (buf * BM + lr + 32 * i) * LDK + kc * 4) = xr[i];
#pragma unroll
        for (int i = 0; i < WI; ++i)
            if (lr + 32 * i < BN)
                *(f32x4 *)(sW + (buf * BN + lr + 32 * i) * LDK + kc * 4) = wr[i];
    };

    // ---- MFMA role
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l15 = lane & 15, quad = lane >> 4;
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    BlockTotal tot[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) tot[i][j].clear();
    if (kt0 < kt1) {
        load_tile(kt0);
        store_tile(0);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        const bool more = kt + 1 < kt1;
        if (more && DBG < 1) load_tile(kt + 1);
        const float *cX = sX + (cur * BM + wm * TM * 16 + l15) * LDK + quad * 4;
        const float *cW = sW + (cur * BN + wn * TN * 16 + l15) * LDK + quad * 4;
        if (((kt - kt0) & 1) == 0) {                  // a block = two 32-deep k-tiles (blocked_mma above)
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) tot[i][j].add(acc[i][j]);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            f32x4 wf[TN], xf[TM];
#pragma unroll
            for (int i = 0; i < TN; ++i) wf[i] = DBG < 2 ? *(const f32x4 *)(cW + i * 16 * LDK + r * 16) : f32x4{1.f + kt, 2.f, 3.f, 4.f + i};
#pragma unroll
            for (int j = 0; j < TM; ++j) xf[j] = DBG < 2 ? *(const f32x4 *)(cX + j * 16 * LDK + r * 16) : f32x4{1.f, 2.f + kt, 3.f + j, 4.f};
            f32x4 unused = {0.f, 0.f, 0.f, 0.f};
            blocked_mma<TN, TM, false>(acc, unused, wf, xf, r == 0 && ((kt - kt0) & 1) == 0);
        }
        if (more && DBG < 1) store_tile(cur ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) { tot[i][j].add(acc[i][j]); acc[i][j] = tot[i][j].get(); }

    // ---- epilogue: lane holds channels co..co+3 (quad*4 + reg) of pixel m (l15)
    if (p.ksplit > 1) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            if (m >= p.M) continue;
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
                const long el = ((long)(ks * p.groups + g) * p.M + m) * p.Cout + co;
                if (co + 3 < p.Cout && (p.Cout & 3) == 0) {
                    ws_store4(p, el, acc[i][j]);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) ws_store1(p, el + e, acc[i][j][e]);
                }
            }
        }
        if (p.combine) splitk_combine<BM, BN>(p, g, t, tiles, bm0, bn0, tid, (int *)smem);
        return;
    }
    const float *__restrict__ bg = p.bias ? p.bias + (long)g * p.b_gs : nullptr;
    const float *__restrict__ rg = p.res ? p.res + (long)g * p.r_gs : nullptr;
    float *__restrict__ yg = p.y + (long)g * p.y_gs;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int m = bm0 + (wm * TM + j) * 16 + l15;
        if (m >= p.M) continue;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
            if (co >= p.Cout) continue;
            f32x4 v = acc[i][j];
            if (p.vec_store && co + 3 < p.Cout) {
                if (bg) v += *(const f32x4 *)(bg + co);
                if (rg) v += *(const f32x4 *)(rg + (long)m * p.res_cstride + p.res_coff + co);
                const int a = co < p.act_split ? p.act : p.act2;
                if (a != USOT_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a);
                }
                *(f32x4 *)(yg + (long)m * p.y_cstride + p.y_coff + co) = v;
            } else {
                const int n = m / p.P, pix = m - n * p.P;
                for (int e = 0; e < 4; ++e) {
                    const int c = co + e;
                    if (c >= p.Cout) break;
                    float s = v[e];
                    if (bg) s += bg[c];
                    if (rg) s += rg[(long)m * p.res_cstride + p.res_coff + c];
                    s = apply_act(s, c < p.act_split ? p.act : p.act2);
                    if (p.y_nchw) yg[((long)n * p.Cout + c) * p.P + pix] = s;
                    else          yg[(long)m * p.y_cstride + p.y_coff + c] = s;
                }
            }
        }
    }
}

}  // namespace
