// Gradients of the fp32 convolution of usot_conv_desc (forward: conv_igemm.hip), same layouts: x NHWC [N][H][W][Cin], dy dense NHWC
// [N][OH][OW][Cout], filter bank w[Cout][K], K = KH*KW*Cin, k = (kh*KW + kw)*Cin + ci; taps outside x contribute 0.
//
//   dw[co][k]       = sum_m dy[m][co] * xcol[m][k]        m = (n, oh, ow),  xcol[m][k] = x[n][oh*s - ph + kh*dh][ow*s - pw + kw*dw][ci]
//   db[co]          = sum_m dy[m][co]
//   dx[n][h][w][ci] = sum_{co, kh, kw : (h + ph - kh*dh) % s == 0, ...} dy[n][(h + ph - kh*dh)/s][(w + pw - kw*dw)/s][co] * w[co][k]
//
// (1) conv_wgrad_f32: a GEMM whose reduction axis is the pixel index, on v_mfma_f32_16x16x4_f32 (exact fp32, a pixel-ordered fmaf
//     chain).  In NHWC both operands are contiguous along the axis that is NOT reduced, so a lane's A value is dy[pixel l>>4][co l&15]
//     and its B value x_tap[pixel l>>4][ci l&15]: whole rows are staged and read back with ds_read_b32, no transpose.  A workgroup
//     (4 wavefronts) owns a 64 (co) x 32 (k) tile of dw - Cin % 32 == 0 keeps the k block inside one tap, so the loader's tap
//     arithmetic is per workgroup - and one of `psplit` slices of the pixel range, [M*s/psplit, M*(s+1)/psplit).  It walks its
//     slice in chunks of 32 pixels (register-staged double buffering, one barrier per chunk, as conv_igemm_f32); wavefront v owns
//     rows 16v .. 16v+15 of the tile and both 16-wide k halves: two independent accumulators.  Rows of LDS are padded by 16 floats
//     (80 / 48): the four pixels a wavefront reads at once then start 16 banks apart and the read is conflict-free.
//     Blocked accumulation as on the forward path: a chunk's 32 products go into a fresh accumulator (first MFMA takes C = 0) and
//     finished chunks into a running total, so chains are 32 + M/(32 psplit) long, not M/psplit.
//     psplit == 1: the workgroup stores its tile of dw.  psplit > 1: it stores the partial tile to slab s of ws[psplit][Cout][K]
//     and conv_wgrad_reduce_f32, a second launch (the kernel boundary is the synchronisation), sums the slabs in slice order.
//     db: the workgroups of k block 0 hold every dy row of their slice and channel block in LDS anyway; their first wavefront
//     sums the columns (rows ascending inside a chunk, then chunks ascending) and the partial sums take the same route through
//     ws[psplit*Cout*K + s*Cout + co].
//     No atomics, no memset, every element of dw / db written once by a plain store, order of summation fixed by (M, psplit).
// (2) conv_pack_dgrad_f32: wt[ci][(kh*KW + kw)*Cout + co] = w[co][((KH-1-kh)*KW + (KW-1-kw))*Cin + ci], the bank rotated by 180
//     degrees and transposed.  With stride 1, dx is the forward convolution of dy with wt at pad' = dil*(K-1) - pad: route A of
//     usot_conv2d_dgrad_f32 hands exactly that descriptor to usot_conv2d_f32.
// (3) conv_dgrad_direct_f32 (route B): one thread per four channels of one dx pixel gathers the dy pixels that reach it.  Any
//     stride, any Cout.  Sums per (tap, 64 output channels) are formed apart and added to the total.  Correctness first: it
//     serves the thin prediction heads (0.4 % of a tower's FLOPs) and strided convolutions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "usot_hip.h"
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BCO = 64, BKK = 32, CHUNK = 32;        // tile of dw (channels x k) and pixels staged per step
constexpr int LDY = BCO + 16, LDX = BKK + 16;        // padded LDS rows (floats)

struct GradK {
    const float *x, *w, *dy;
    float *out;                 // wgrad: dw (psplit == 1) or the slabs;  dgrad / pack: dx / wt
    float *bout;                // wgrad: db (psplit == 1) or the db partials behind the slabs; nullptr = no db
    int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad_h, pad_w, dil_h, dil_w;
    int M, K, P, psplit, KB, CB;
};

__global__ __launch_bounds__(256) void conv_wgrad_f32(const GradK p)
{
    __shared__ __attribute__((aligned(16))) float smem[2 * CHUNK * (LDY + LDX)];     // [buffer][dy rows | x rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, quad = lane >> 4;
    int b = blockIdx.x;
    const int kb = b % p.KB;
    b /= p.KB;
    const int cb = b % p.CB, s = b / p.CB;
    const int k0 = kb * BKK, co0 = cb * BCO;
    const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int m0 = (int)((long)p.M * s / p.psplit), m1 = (int)((long)p.M * (s + 1) / p.psplit);
    const bool cvec = (p.Cout & 3) == 0;

    // loader roles: x - thread (row t >> 3, 16-byte piece t & 7); dy - thread (rows t >> 4 and + 16, channels 4 (t & 15) ..)
    const int xrow = tid >> 3, xc = (tid & 7) * 4;
    const int yrow = tid >> 4, yc = (tid & 15) * 4;
    f32x4 xr, yr[2];
    auto load_chunk = [&](int mb) {
        {
            const int m = mb + xrow;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m1) {
                const int n = m / p.P, pix = m - n * p.P;
                const int oh = pix / p.OW, ow = pix - oh * p.OW;
                const int ih = oh * p.stride - p.pad_h + kh * p.dil_h, iw = ow * p.stride - p.pad_w + kw * p.dil_w;
                if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
                    v = *(const f32x4 *)(p.x + (((long)n * p.H + ih) * p.W + iw) * p.Cin + c0 + xc);
            }
            xr = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = mb + yrow + 16 * i, co = co0 + yc;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m1) {
                const float *src = p.dy + (long)m * p.Cout + co;
                if (cvec) {
                    if (co < p.Cout) v = *(const f32x4 *)src;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) v[e] = src[e];
                }
            }
            yr[i] = v;
        }
    };
    auto store_chunk = [&](int buf) {
        float *sy = smem + buf * CHUNK * (LDY + LDX), *sx = sy + CHUNK * LDY;
        *(f32x4 *)(sx + xrow * LDX + xc) = xr;
        *(f32x4 *)(sy + yrow * LDY + yc) = yr[0];
        *(f32x4 *)(sy + (yrow + 16) * LDY + yc) = yr[1];
    };

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc0 = zero, acc1 = zero;
    BlockTotal tot0, tot1;
    tot0.clear();
    tot1.clear();
    const bool want_b = p.bout != nullptr && kb == 0 && tid < BCO;       // wavefront 0 of the k block 0 workgroups
    float btot = 0.f;

    load_chunk(m0);
    store_chunk(0);
    __syncthreads();
    int cur = 0;
    for (int mb = m0; mb < m1; mb += CHUNK) {
        const bool more = mb + CHUNK < m1;
        if (more) load_chunk(mb + CHUNK);
        const float *sy = smem + cur * CHUNK * (LDY + LDX), *sx = sy + CHUNK * LDY;
        tot0.add(acc0);
        tot1.add(acc1);
        const float *ay = sy + quad * LDY + wave * 16 + l15, *ax = sx + quad * LDX + l15;
#pragma unroll
        for (int j = 0; j < CHUNK / 4; ++j) {
            const float a = ay[j * 4 * LDY], b0 = ax[j * 4 * LDX], b1 = ax[j * 4 * LDX + 16];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, j == 0 ? zero : acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, j == 0 ? zero : acc1, 0, 0, 0);
        }
        if (want_b) {
            float c = 0.f;
#pragma unroll 8
            for (int r = 0; r < CHUNK; ++r) c += sy[r * LDY + tid];
            btot += c;
        }
        if (more) store_chunk(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    tot0.add(acc0);
    tot1.add(acc1);
    acc0 = tot0.get();
    acc1 = tot1.get();

    // lane holds rows co0 + 16 wave + 4 quad + e (e = 0 .. 3) of columns k0 + l15 and k0 + 16 + l15
    float *dst = p.out + (long)s * p.Cout * p.K;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int co = co0 + wave * 16 + quad * 4 + e;
        if (co < p.Cout) {
            dst[(long)co * p.K + k0 + l15] = acc0[e];
            dst[(long)co * p.K + k0 + 16 + l15] = acc1[e];
        }
    }
    if (want_b && co0 + tid < p.Cout) p.bout[(long)s * p.Cout + co0 + tid] = btot;
}

// dw[i] = sum_s slab[s][i] (s ascending), four floats per thread; behind them db[c] = sum_s part[s][c]
__global__ __launch_bounds__(256) void conv_wgrad_reduce_f32(const float *__restrict__ ws, float *__restrict__ dw, float *__restrict__ db,
                                                            long n4, int Cout, int psplit)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < n4) {
        const f32x4 *src = (const f32x4 *)ws + idx;
        f32x4 v = src[0];
        for (int s = 1; s < psplit; ++s) v += src[(long)s * n4];
        ((f32x4 *)dw)[idx] = v;
    } else if (db && idx < n4 + Cout) {
        const int c = (int)(idx - n4);
        const float *src = ws + n4 * 4 * psplit + c;
        float v = src[0];
        for (int s = 1; s < psplit; ++s) v += src[(long)s * Cout];
        db[c] = v;
    }
}

__global__ __launch_bounds__(256) void conv_pack_dgrad_kernel(const float *__restrict__ w, float *__restrict__ wt,
                                                             int Cout, int Cin, int T, long total)
{
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int co = (int)(idx % Cout);
        const int tp = (int)((idx / Cout) % T);
        const int ci = (int)(idx / ((long)Cout * T));
        wt[idx] = w[((long)co * T + (T - 1 - tp)) * Cin + ci];
    }
}

__global__ __launch_bounds__(256) void conv_dgrad_direct_f32(const GradK p)
{
    const int c4n = p.Cin >> 2;
    const long total = (long)p.N * p.H * p.W * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int ci = (int)(idx % c4n) * 4;
        const long pix = idx / c4n;
        const int wq = (int)(pix % p.W);
        const int hq = (int)((pix / p.W) % p.H);
        const int n = (int)(pix / ((long)p.W * p.H));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kh = 0; kh < p.KH; ++kh) {
            const int th = hq + p.pad_h - kh * p.dil_h;
            if (th < 0 || th % p.stride) continue;
            const int oh = th / p.stride;
            if (oh >= p.OH) continue;
            for (int kw = 0; kw < p.KW; ++kw) {
                const int tw = wq + p.pad_w - kw * p.dil_w;
                if (tw < 0 || tw % p.stride) continue;
                const int ow = tw / p.stride;
                if (ow >= p.OW) continue;
                const float *dyp = p.dy + (((long)n * p.OH + oh) * p.OW + ow) * p.Cout;
                const float *wp = p.w + (long)(kh * p.KW + kw) * p.Cin + ci;
                for (int cb = 0; cb < p.Cout; cb += 64) {
                    const int ce = cb + 64 < p.Cout ? cb + 64 : p.Cout;
                    f32x4 t = {0.f, 0.f, 0.f, 0.f};
                    for (int co = cb; co < ce; ++co) {
                        const float d = dyp[co];
                        const f32x4 wv = *(const f32x4 *)(wp + (long)co * p.K);
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = fmaf(d, wv[e], t[e]);
                    }
                    acc += t;
                }
            }
        }
        *(f32x4 *)(p.out + idx * 4) = acc;
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

// what both launchers check before they touch the device (and the host-only queries, for their answer to mean something)
int grad_geometry_ok(const usot_conv_grad_desc *d)
{
    if (!d) return 0;
    if (d->N < 0 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->OH < 1 || d->OW < 1 || d->Cout < 1) return 0;
    if (d->KH < 1 || d->KW < 1 || d->stride < 1 || d->pad_h < 0 || d->pad_w < 0 || d->dil_h < 1 || d->dil_w < 1) return 0;
    if (d->Cin & 31) return 0;
    const long eh = (long)d->H + 2L * d->pad_h - (long)d->dil_h * (d->KH - 1) - 1;
    const long ew = (long)d->W + 2L * d->pad_w - (long)d->dil_w * (d->KW - 1) - 1;
    if (eh < 0 || ew < 0 || eh / d->stride + 1 != d->OH || ew / d->stride + 1 != d->OW) return 0;
    // 32-bit pixel and filter indices in the kernels
    if ((long)d->N * d->OH * d->OW >= (1L << 31) || (long)d->N * d->H * d->W >= (1L << 31)) return 0;
    if ((long)d->KH * d->KW * d->Cin * d->Cout >= (1L << 31)) return 0;
    return 1;
}

int wgrad_auto_psplit(const usot_conv_grad_desc *d)
{
    const long M = (long)d->N * d->OH * d->OW;
    const long tiles = (long)((d->Cout + BCO - 1) / BCO) * (d->KH * d->KW * d->Cin / BKK);
    long ps = (4L * device_cus() + tiles - 1) / tiles;           // four workgroups per CU (32 KB of LDS each: five fit) ...
    const long most = M / (2 * CHUNK);                           // ... but no slice below two pixel chunks
    if (ps > most) ps = most;
    if (ps > 32) ps = 32;
    return ps < 1 ? 1 : (int)ps;
}

void fill_grad(const usot_conv_grad_desc *d, GradK &p)
{
    p.x = d->x; p.w = d->w; p.dy = d->dy;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad_h = d->pad_h; p.pad_w = d->pad_w; p.dil_h = d->dil_h; p.dil_w = d->dil_w;
    p.P = d->OH * d->OW;
    p.M = d->N * p.P;
    p.K = d->KH * d->KW * d->Cin;
    p.KB = p.K / BKK;
    p.CB = (d->Cout + BCO - 1) / BCO;
    p.psplit = 1;
    p.out = p.bout = nullptr;
}

// route A is open to: stride 1, whole 32-channel blocks of dy, a rotated bank, and a pad' = dil*(K-1) - pad that is a padding
bool route_a_eligible(const usot_conv_grad_desc *d)
{
    return d->stride == 1 && (d->Cout & 31) == 0 && d->wt != nullptr &&
           d->dil_h * (d->KH - 1) - d->pad_h >= 0 && d->dil_w * (d->KW - 1) - d->pad_w >= 0;
}

}  // namespace

extern "C" int usot_conv2d_wgrad_geometry(int *bco, int *bk, int *chunk)
{
    if (bco) *bco = BCO;
    if (bk) *bk = BKK;
    if (chunk) *chunk = CHUNK;
    return USOT_OK;
}

extern "C" int usot_conv2d_wgrad_psplit(const usot_conv_grad_desc *d)
{
    if (!grad_geometry_ok(d) || d->psplit < 0) return USOT_EINVAL;
    if (d->psplit > 0) return d->psplit;
    return d->N == 0 ? 1 : wgrad_auto_psplit(d);
}

extern "C" int64_t usot_conv2d_wgrad_ws_floats(const usot_conv_grad_desc *d)
{
    const int ps = usot_conv2d_wgrad_psplit(d);
    if (ps < 0) return ps;
    if (ps == 1) return 0;
    return (int64_t)ps * d->Cout * ((int64_t)d->KH * d->KW * d->Cin + 1);     // slabs [ps][Cout][K], then db partials [ps][Cout]
}

extern "C" int usot_conv2d_wgrad_f32(void *stream, const usot_conv_grad_desc *d)
{
    if (!grad_geometry_ok(d) || !d->x || !d->dy || !d->dw || d->psplit < 0) return USOT_EINVAL;
    if (((uintptr_t)d->x | (uintptr_t)d->dy | (uintptr_t)d->dw | (uintptr_t)d->ws) & 15) return USOT_EINVAL;
    if (d->N == 0) return USOT_OK;
    GradK p;
    fill_grad(d, p);
    if (d->psplit > p.M) return USOT_EINVAL;
    const int ps = d->psplit > 0 ? d->psplit : wgrad_auto_psplit(d);
    if (ps > 1 && !d->ws) return USOT_EINVAL;
    const long blocks = (long)p.KB * p.CB * ps;
    if (blocks > 0x7fffffffL) return USOT_EINVAL;
    const long slab = (long)p.Cout * p.K;
    p.psplit = ps;
    p.out = ps == 1 ? d->dw : d->ws;
    p.bout = !d->db ? nullptr : (ps == 1 ? d->db : d->ws + slab * ps);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_wgrad_f32, dim3((unsigned)blocks), dim3(256), 0, s, p);
    USOT_CHECK_LAUNCH();
    if (ps > 1) {
        const long n4 = slab / 4;
        hipLaunchKernelGGL(conv_wgrad_reduce_f32, dim3((unsigned)usot_cdiv(n4 + p.Cout, 256)), dim3(256), 0, s,
                           (const float *)d->ws, d->dw, d->db, n4, p.Cout, ps);
        USOT_CHECK_LAUNCH();
    }
    return USOT_OK;
}

extern "C" int usot_conv_pack_dgrad_f32(void *stream, const float *w, float *wt, int Cout, int Cin, int KH, int KW)
{
    if (!w || !wt || Cout < 1 || Cin < 1 || KH < 1 || KW < 1) return USOT_EINVAL;
    const long total = (long)Cout * Cin * KH * KW;
    if (total >= (1L << 31)) return USOT_EINVAL;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(conv_pack_dgrad_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       w, wt, Cout, Cin, KH * KW, total);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_conv2d_dgrad_route(const usot_conv_grad_desc *d)
{
    if (!grad_geometry_ok(d) || d->route < 0 || d->route > 2) return USOT_EINVAL;
    if (d->route == 2) return 2;
    if (route_a_eligible(d)) return 1;
    return d->route == 1 ? USOT_EINVAL : 2;
}

extern "C" int usot_conv2d_dgrad_f32(void *stream, const usot_conv_grad_desc *d)
{
    if (!grad_geometry_ok(d) || !d->dy || !d->w || !d->dx) return USOT_EINVAL;
    const int route = usot_conv2d_dgrad_route(d);
    if (route < 0) return route;
    if (((uintptr_t)d->dy | (uintptr_t)d->w | (uintptr_t)d->dx) & 15) return USOT_EINVAL;
    if (d->N == 0) return USOT_OK;
    if (route == 1) {
        usot_conv_desc f = {};
        f.x = d->dy; f.w = d->wt; f.y = d->dx;
        f.N = d->N; f.H = d->OH; f.W = d->OW; f.Cin = d->Cout; f.OH = d->H; f.OW = d->W; f.Cout = d->Cin;
        f.KH = d->KH; f.KW = d->KW; f.stride = 1;
        f.pad_h = d->dil_h * (d->KH - 1) - d->pad_h; f.pad_w = d->dil_w * (d->KW - 1) - d->pad_w;
        f.dil_h = d->dil_h; f.dil_w = d->dil_w;
        f.groups = 1; f.ksplit = 1;
        const int rc = usot_conv2d_f32(stream, &f);
        if (rc != USOT_EINVAL || d->route == 1) return rc;         // a geometry the forward launcher does not take: route B
    }
    GradK p;
    fill_grad(d, p);
    p.out = d->dx;
    const long blocks = ((long)p.N * p.H * p.W * (p.Cin / 4) + 255) / 256;
    hipLaunchKernelGGL(conv_dgrad_direct_f32, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, p);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}
