// What every fp32 convolution kernel generation shares (conv_f32_v1.h, _v2.h, _v3.h and the lab/ headers; the overview of the GEMM
// view and the tiling heads conv_igemm.hip, which includes all of them): the kernel-side problem block ConvK and the batch of up to
// four of them, the activation epilogue, the split-K slab stores and in-launch combine, the XCD block remap and blocked_mma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "usot_hip.h"
#include "common.h"
#include "fastdiv.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// What a kernel reads between its entry and its first k-step, in ONE contiguous block of five 64-byte lines at the front of a problem:
// the kernels fetch it with five s_load_dwordx16 issued together and waited for once (conv_pro_fetch below) instead of a field at a
// time where each is first used - ten dependent scalar-memory round trips in front of the first activation load on the parent of
// this layout (docs/LAB_NOTEBOOK.md A.9).  fill_params and the launcher fill it, the division constants (fastdiv.h) included: every
// quotient of the index prologue has a divisor that is known when the launch is prepared.
struct alignas(64) ConvPro {
    const float *x, *w, *bias, *res;
    float *y, *ws;
    const int *n_dyn;                   // v3 tiles: nullptr, or a device word with a run-time image count (usot_conv_desc.n_dyn): images
                                        // [0, clamp(*n_dyn - n_first, 0, N)) of this problem are live, the rest is neither read nor written
    const float *wscale;                // split-fp16 tiles (PF = 4): 1 / (filter row scale x activation scale) per output channel
    long x_gs, w_gs, b_gs, y_gs, r_gs;
    int N, H, W, Cin, OW, Cout;
    int stride, pad_h, pad_w, dil_h, dil_w, KW;
    int P, M, K;                        // P = OH*OW
    int ktb, cch;                       // k-tiles of the launched tile: K / bk in all, Cin / bk per filter tap
    int ksplit, groups, n_first, MT, NT;
    int tiles, total;                   // MT * NT; tiles * groups * ksplit = the problem's workgroups
    FastDiv d_tiles, d_ksplit, d_MT, d_P, d_OW, d_KW, d_cch;
    int vec_store, res_cstride, res_coff, KH, OH;
};
static_assert(sizeof(ConvPro) == 320, "five 64-byte lines");

struct ConvK : ConvPro {
    int y_cstride, y_coff, y_nchw;
    int act, act2, act_split;
    int combine;                        // split-K: 1 = last-arriver combine inside the launch, 0 = second launch
    int KT, cchunks;                    // k-tiles of 32 (v1 and the lab families)
    int pr;                             // weight-stationary tiles: pixel ranges per (group, 32-channel block)
    const float *zero;                  // PF = 6: 16 zero bytes, the source of padding taps for the activation DMA
    int x_split, y_split;               // the input map arrives / the result leaves in the split-fp16 layout (usot_conv_desc)
    int *ovf;                           // split-fp16 tiles: sticky "a finished sum was not finite" word (usot_conv_desc.ovf) or nullptr
};

// Up to four convolutions of DIFFERENT geometry in one launch (same tile shape): the shortcut
// conv beside conv1 of a bottleneck, the three dilated encoders of one input, the two
// prediction heads.  At batch 1 each of these alone leaves most of the chip idle and pays a
// full launch; side by side they share one.  Workgroup ranges are [start[i], start[i+1]).
// n and start[] stand in front: the first scalar fetch of a kernel, which selects the problem.
struct ConvBatch {
    int n;
    int start[5];
    int pad_[2];
    ConvK p[4];
};
constexpr int kBatchHead = 64;          // bytes in front of p[0]
static_assert(sizeof(ConvBatch) == kBatchHead + 4 * sizeof(ConvK) && sizeof(ConvK) % 64 == 0, "problem blocks on 64-byte lines");

// The prologue fetch.  ConvBatch is the FIRST kernel argument of every conv kernel, so it stands at offset 0 of the kernel-argument
// segment; reading it through the segment pointer (constant address space, uniform address) gives wide scalar loads that the
// compiler can neither split nor sink to the fields' uses.  Two dependent rounds for a single-problem launch, three for a batch:
//   1. n, start[] AND problem 0's block, issued together, one wait;
//   2. only where the workgroup belongs to problem 1-3: that problem's block;
//   3. the caller's *n_dyn.
// The empty asm carries the values through SGPRs: behind it they are registers, not re-loadable kernel arguments.
typedef uint32_t u32x16_t __attribute__((ext_vector_type(16)));
typedef uint32_t u32x8_t __attribute__((ext_vector_type(8)));
struct ConvProBits { u32x16_t v[5]; };
static_assert(sizeof(ConvProBits) == sizeof(ConvPro), "bit image of the prologue block");
#define USOT_KARG __attribute__((address_space(4)))
__device__ __forceinline__ ConvPro conv_pro_fetch(int &pi, int &bid0)
{
    const USOT_KARG char *ka = (const USOT_KARG char *)__builtin_amdgcn_kernarg_segment_ptr();
    u32x8_t hd = *(const USOT_KARG u32x8_t *)ka;
    const USOT_KARG u32x16_t *b0 = (const USOT_KARG u32x16_t *)(ka + kBatchHead);
    u32x16_t v0 = b0[0], v1 = b0[1], v2 = b0[2], v3 = b0[3], v4 = b0[4];
    asm volatile("" : "+s"(hd), "+s"(v0), "+s"(v1), "+s"(v2), "+s"(v3), "+s"(v4));
    const int n = (int)hd[0];
    pi = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (q < n && (int)blockIdx.x >= (int)hd[1 + q]) pi = q;
    bid0 = (int)blockIdx.x - (pi == 0 ? (int)hd[1] : pi == 1 ? (int)hd[2] : pi == 2 ? (int)hd[3] : (int)hd[4]);
    if (pi != 0) {
        const USOT_KARG u32x16_t *bp = (const USOT_KARG u32x16_t *)(ka + kBatchHead + (size_t)pi * sizeof(ConvK));
        v0 = bp[0]; v1 = bp[1]; v2 = bp[2]; v3 = bp[3]; v4 = bp[4];
        asm volatile("" : "+s"(v0), "+s"(v1), "+s"(v2), "+s"(v3), "+s"(v4));
    }
    const ConvProBits bits = {{v0, v1, v2, v3, v4}};
    ConvPro q = __builtin_bit_cast(ConvPro, bits);
    // pointers that come out of a bit image are generic to the compiler (flat_load: counted on lgkmcnt too, which would tie the
    // producers' loads to the LDS waits); kernel arguments point to global memory, and through these casts it knows again
#define USOT_GLOBAL_PTR(f) q.f = (decltype(q.f))(__attribute__((address_space(1))) void *)(uintptr_t)q.f
    USOT_GLOBAL_PTR(x); USOT_GLOBAL_PTR(w); USOT_GLOBAL_PTR(bias); USOT_GLOBAL_PTR(res);
    USOT_GLOBAL_PTR(y); USOT_GLOBAL_PTR(ws); USOT_GLOBAL_PTR(n_dyn); USOT_GLOBAL_PTR(wscale);
#undef USOT_GLOBAL_PTR
    return q;
}
__device__ __forceinline__ int fd_div(int n, FastDiv f) { return (int)fastdiv_div((uint32_t)n, f); }

__device__ __forceinline__ float apply_act(float v, int a)
{
    switch (a) {
    case USOT_ACT_RELU: return fmaxf(v, 0.0f);
    case USOT_ACT_EXP:  return expf(v);
    case USOT_ACT_CONF: return expf(fminf(fmaxf(v, 0.0f), 4.0f));
    default:            return v;
    }
}

// write-through (sc1) slab accesses through a buffer descriptor: the partial tiles of a split-K launch bypass the
// issuing CU's L1 and are not left dirty in its XCD's L2, so the hand-off needs NO release fence (buffer_wbl2 writes
// back the whole L2 slice: 1.7-6.5 us) and the reader no acquire (cdna_hip_programming.md Guideline 16, recipe R1)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ws_rsrc(const ConvK &p)
{
    const long bytes = ((long)p.ksplit * p.groups * p.M * p.Cout) * 4;
    return __builtin_amdgcn_make_buffer_rsrc((void *)p.ws, 0, (int)(bytes > 0x7fffffffL ? 0x7fffffffL : bytes), 0x00020000);
}
__device__ __forceinline__ void ws_store4(const ConvK &p, long elem, f32x4 v)
{
    if (p.combine) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), ws_rsrc(p), (int)(elem * 4), 0, 16);
    else           *(f32x4 *)(p.ws + elem) = v;
}
__device__ __forceinline__ void ws_store1(const ConvK &p, long elem, float v)
{
    if (p.combine) __hip_atomic_store(p.ws + elem, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else           p.ws[elem] = v;
}

// In-launch split-K combine.  Every k-slice workgroup has stored its partial tile to the workspace slab
// [ks][group][M][Cout]; the LAST slice to arrive (one ticket per tile) sums the slabs in slice order — the
// same order, hence the same bits, whichever workgroup does it — and applies bias / residual / activation.
// Replaces the separate reduction launch (4.8 us + a kernel boundary per split layer at batch 1).
// Protocol (cdna_hip_programming.md, Guideline 16 recipe R1 / "in-launch split-K reduction"): write-through (sc1)
// slab stores -> every wave drains vmcnt -> barrier -> ONE lane: relaxed agent-scope fetch_add -> last arriver:
// barrier -> sc1 slab loads.  No fences (the release form, buffer_wbl2, measured 14 us per frame SLOWER than the
// separate reduction launch it replaces).  Placement-independent.  The ticket words live
// behind the slabs, are zero before the first launch (the engine zero-fills the workspace) and are reset by
// the last arriver, so every launch — and every graph replay — finds them zero.
template <int BM, int BN>
__device__ __forceinline__ void splitk_combine(const ConvK &p, int g, int t0, int tiles, int bm0, int bn0, int tid, int *flag, int mlim = -1)
{
    const int ML = mlim < 0 ? p.M : mlim;     // rows the launch computes (n_dyn: fewer than M; slab strides and tickets keep the static M)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        int *cnt = (int *)(p.ws + (long)p.ksplit * p.groups * p.M * p.Cout) + (g * tiles + t0);
        const int ticket = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == p.ksplit - 1;
        if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    const float *__restrict__ bg = p.bias ? p.bias + (long)g * p.b_gs : nullptr;
    const float *__restrict__ rg = p.res ? p.res + (long)g * p.r_gs : nullptr;
    float *__restrict__ yg = p.y + (long)g * p.y_gs;
    const long slab = (long)p.groups * p.M * p.Cout;
    const float *ws0 = p.ws + (long)g * p.M * p.Cout;
    const __amdgpu_buffer_rsrc_t rs = ws_rsrc(p);
    if (p.vec_store && (p.Cout & 3) == 0) {
        for (int idx = tid; idx < BM * (BN / 4); idx += 256) {
            const int row = idx / (BN / 4), c4 = (idx - row * (BN / 4)) * 4;
            const int m = bm0 + row, co = bn0 + c4;
            if (m >= ML || co >= p.Cout) continue;
            const long el = (long)g * p.M * p.Cout + (long)m * p.Cout + co;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < p.ksplit; ++ks)
                v += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((el + ks * slab) * 4), 0, 16));
            if (bg) v += *(const f32x4 *)(bg + co);
            if (rg) v += *(const f32x4 *)(rg + (long)m * p.res_cstride + p.res_coff + co);
            const int a = co < p.act_split ? p.act : p.act2;
            if (a != USOT_ACT_NONE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a);
            }
            *(f32x4 *)(yg + (long)m * p.y_cstride + p.y_coff + co) = v;
        }
        return;
    }
    for (int idx = tid; idx < BM * BN; idx += 256) {
        const int row = idx / BN, cc = idx - row * BN;
        const int m = bm0 + row, c = bn0 + cc;
        if (m >= ML || c >= p.Cout) continue;
        float sum = 0.f;
        for (int ks = 0; ks < p.ksplit; ++ks) sum += __hip_atomic_load(ws0 + ks * slab + (long)m * p.Cout + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bg) sum += bg[c];
        if (rg) sum += rg[(long)m * p.res_cstride + p.res_coff + c];
        sum = apply_act(sum, c < p.act_split ? p.act : p.act2);
        if (p.y_nchw) {
            const int n = m / p.P, pix = m - n * p.P;
            yg[((long)n * p.Cout + c) * p.P + pix] = sum;
        } else {
            yg[(long)m * p.y_cstride + p.y_coff + c] = sum;
        }
    }
}

// XCD-aware, bijective block remap: the dispatcher places block b on XCD b % 8; give each
// XCD a contiguous chunk of the tile space so the M-tiles that share a weight strip (and
// the neighbouring pixels' input rows) meet in one L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int total)
{
    const int q = total >> 3, r = total & 7;
    const int xcd = b & 7, idx = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

constexpr int LDK = 36;   // padded k-extent of an LDS row (floats)
__device__ __attribute__((aligned(16))) uint32_t g_zero16_f32[4] = {0u, 0u, 0u, 0u};     // source of padding taps (activation DMA, PF = 6)

// Blocked accumulation.  v_mfma_f32_16x16x4_f32 adds its four products to C one after the other, so a plain k-loop is ONE
// sequential float32 chain of K additions per output: on a K = 4608 reduction its rounding error is 4x (rms) that of a
// CPU convolution of the same data, and with filters that pass the DC level of post-ReLU maps the frame's logits end up
// 2.8x further from a float64 evaluation than the reference's own float32 arithmetic (tests/test_gpu_model.py, 'dc' family).
// Every fp32 conv kernel therefore sums a k-tile (32 / 64 products) into a fresh accumulator — the first MFMA of a block
// takes C = 0, an inline constant: nothing to clear — and adds finished blocks to a running total (common.h: BlockTotal;
// plain float32 by default, float64 / Kahan forms measured there), eight VALU adds per k-tile placed right after the
// k-loop's barrier where the block's MFMAs have long retired, issued in the shadow of the next block's MFMAs.  Chains:
// 64 + K/64 instead of K.  Emulated on the layer3.0 shortcut conv: rms error of the output 1.76e-6 (single
// chain) -> 3.6e-7 (float32 total; torch-CPU: 3.9e-7); measured on the whole frame in tests/golden/f64_gate.py.
// one 16-k round = 4 MFMAs per 16x16 block from the fragments wf / xf; first: this round starts a block
template <int TN, int TM, bool DUAL = true>
__device__ __forceinline__ void blocked_mma(f32x4 (&acc)[TN][TM], f32x4 &acc2, const f32x4 (&wf)[TN], const f32x4 (&xf)[TM], bool first)
{
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (TM * TN == 1 && DUAL) {
        // a wave with a single 16x16 block alternates two accumulators (40-cycle dependent latency vs 32-cycle issue)
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][0], xf[0][0], first ? zero : acc[0][0], 0, 0, 0);
        acc2      = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][1], xf[0][1], first ? zero : acc2, 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][2], xf[0][2], acc[0][0], 0, 0, 0);
        acc2      = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][3], xf[0][3], acc2, 0, 0, 0);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][c], xf[j][c], (first && c == 0) ? zero : acc[i][j], 0, 0, 0);
    }
}

// Launch geometry: ONE constexpr struct per kernel family, of the kernel's own template parameters.  The kernel reads its launch bounds
// and LDS layout from it and the family's TILE* macro fills the kTiles row (conv_igemm.hip) from it: no other thread count or LDS size anywhere.

}  // namespace
