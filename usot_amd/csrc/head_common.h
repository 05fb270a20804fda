// Device code shared by the single-frame head kernels (head_ops.hip) and their lock-step batched forms (multitrack.hip):
// one copy of the decode (cell scan, argmax, result block, RoI row), of the memory bank's append + gather and of the SiamFC
// crop arithmetic, so that a batched slot is bit-identical to the single-frame kernel run on that slot.  The kernels
// themselves only differ in where their control words come from and in their per-slot offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace usot_head {

// ---- decode (usot_tracker.py:138-163): the state one thread keeps for its best response cell
struct DecCell {
    double ps, x1, y1, x2, y2, pen;
    float sc;
    int i;
};

// np.argmax semantics (usot_tracker.py:163): first maximum, and a NaN counts as the maximum (the first NaN wins);
// index 0x7fffffff = "no cell" loses to everything
__device__ __forceinline__ bool dec_better(double ov, int oi, double mv, int mi)
{
    const bool on = ov != ov, mn = mv != mv;
    return oi != 0x7fffffff &&
        (mi == 0x7fffffff || (on && !mn) || (on == mn && (on ? oi < mi : (ov > mv || (ov == mv && oi < mi)))));
}

// Every cell of one S x S response (cls, cls_mem [n], bbox [4][n], window [n]; n = S * S) against the target size (tw, th):
// one response cell per thread at S <= 32 (a single pass: the loads of all six maps in flight together), the argmax as a
// wavefront butterfly + one LDS round over the waves.  Fills `best` with this thread's best cell and returns whether it is
// the workgroup's: that thread still holds the winner's box, score and penalty in registers and publishes them.  The winner
// is a valid cell whatever the maps hold (every cell beats "no cell").  Called by the whole workgroup (it synchronises).
__device__ __forceinline__ bool dec_scan_argmax(DecCell &best, const float *__restrict__ cls, const float *__restrict__ cls_mem,
                                                const float *__restrict__ bbox, const double *__restrict__ window, int S,
                                                int instance_size, int stride, float ratio, double penalty_k,
                                                double window_influence, double tw, double th)
{
    __shared__ double wave_v[16];
    __shared__ int wave_i[16];
    __shared__ int win_i;
    const int n = S * S;
    const double tpad = (tw + th) * 0.5;
    const double tsz = sqrt((tw + tpad) * (th + tpad));
    const double tratio = tw / th;
    best.ps = -1e300; best.i = 0x7fffffff;
    best.x1 = best.y1 = best.x2 = best.y2 = best.pen = 0.0; best.sc = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = i / S, c = i - r * S;
        const double gx = (double)((c - S / 2) * stride + instance_size / 2);
        const double gy = (double)((r - S / 2) * stride + instance_size / 2);
        const float s0 = 1.0f / (1.0f + expf(-cls[i]));
        const float s1 = 1.0f / (1.0f + expf(-cls_mem[i]));
        const float sc = ratio * s0 + (1.0f - ratio) * s1;
        const double x1 = gx - (double)bbox[i], y1 = gy - (double)bbox[n + i];
        const double x2 = gx + (double)bbox[2 * n + i], y2 = gy + (double)bbox[3 * n + i];
        const double w = x2 - x1, h = y2 - y1;
        const double pad = (w + h) * 0.5;
        double sr = sqrt((w + pad) * (h + pad)) / tsz;
        sr = fmax(sr, 1.0 / sr);
        double rr = tratio / (w / h);
        rr = fmax(rr, 1.0 / rr);
        const double pen = exp(-(rr * sr - 1.0) * penalty_k);
        const double ps = pen * (double)sc * (1.0 - window_influence) + window[i] * window_influence;
        if (dec_better(ps, i, best.ps, best.i)) {
            best.ps = ps; best.i = i; best.sc = sc; best.pen = pen;
            best.x1 = x1; best.y1 = y1; best.x2 = x2; best.y2 = y2;
        }
    }
    double rv = best.ps;
    int ri = best.i;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(rv, off, 64);
        const int oi = __shfl_xor(ri, off, 64);
        if (dec_better(ov, oi, rv, ri)) { rv = ov; ri = oi; }
    }
    const int wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { wave_v[wv] = rv; wave_i[wv] = ri; }
    __syncthreads();
    if (threadIdx.x < 64) {
        rv = threadIdx.x < nw ? wave_v[threadIdx.x] : -1e300;
        ri = threadIdx.x < nw ? wave_i[threadIdx.x] : 0x7fffffff;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const double ov = __shfl_xor(rv, off, 64);
            const int oi = __shfl_xor(ri, off, 64);
            if (dec_better(ov, oi, rv, ri)) { rv = ov; ri = oi; }
        }
        if (threadIdx.x == 0) win_i = ri;
    }
    __syncthreads();
    return best.i == win_i;
}

// The winning thread's results: out[0 .. 7], and with `roi` the PrRoIPool row of the best box, roi[0] = roi_batch (0 for a single
// frame, the slot for a batch).  The caller fences and writes its tag behind this.
__device__ __forceinline__ void dec_publish(const DecCell &best, double *__restrict__ out, float *__restrict__ roi, float roi_batch,
                                            int S, int instance_size, int stride)
{
    out[0] = (double)best.i;
    out[1] = (double)best.sc;
    out[2] = best.pen;
    out[3] = best.x1; out[4] = best.y1; out[5] = best.x2; out[6] = best.y2;
    out[7] = best.ps;
    if (!roi) return;
    // usot_tracker.py:329-350 (pool_label_search): the S-point axis of the response map applied to the search feature; box
    // rounded to float32 first (np.array(..., np.float32)), arithmetic in float64, result stored as float32 (.float()).
    const double lo = (double)((0 - S / 2) * stride + instance_size / 2);
    const double hi = (double)((S - 1 - S / 2) * stride + instance_size / 2);
    const double slope = (double)(2 * (S / 2)) / (hi - lo);
    const double gap = 1.0 / slope;
    const double bx[4] = {best.x1, best.y1, best.x2, best.y2};
    roi[0] = roi_batch;
    for (int e = 0; e < 4; ++e) {
        double v = (double)(float)bx[e];
        v = v < lo - gap ? lo - gap : (v > hi + gap ? hi + gap : v);      // np.clip: a NaN stays a NaN (fmax / fmin would drop it)
        roi[1 + e] = (float)((v - lo) * slope);
    }
}

// one thread per response cell up to 1024 cells (S <= 32), whole wavefronts
inline unsigned decode_threads(int S)
{
    const int n = S * S;
    return (unsigned)(n >= 1024 ? 1024 : (n + 63) / 64 * 64);
}

// ---- memory bank, append + gather in ONE launch: the row the PREVIOUS frame pooled (bank 0) and its three encodings (banks
// 1-3) go to row `app` of their banks, and n_pick rows of banks 1-3 are gathered into the frame's picked-kernel buffers - a
// picked row that IS the appended row is read from the fresh row itself, so the two halves need no ordering between them.
// blockIdx.y: 0-3 = append bank y, 4-6 = gather bank y - 3; blockIdx.x strides over a row's (a gather's) 16-byte elements.
// Slot b of a batch owns row b of fresh[] and rows [b * n_pick, (b + 1) * n_pick) of picked[]; a single frame is b = 0.
struct RowsAG {
    const float *fresh[4];
    float *bank[4];
    float *picked[3];
    int row_len4[4];
    int n_pick;
    int arg;           // single frame: the position of the append row in idx[]; batch: the rows of a bank (the range rule)
};

__device__ __forceinline__ void rows_append_row(const RowsAG &k, int job, int app, int b)
{
    const int rl = k.row_len4[job];
    const usot_f32x4 *__restrict__ src = (const usot_f32x4 *)k.fresh[job] + (long)b * rl;
    usot_f32x4 *__restrict__ dst = (usot_f32x4 *)k.bank[job] + (long)app * rl;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < rl; i += gridDim.x * 256) dst[i] = src[i];
}

// n_rows rows of bank g into picked[g - 1]: row r is rows[r], or rows[lead[r]] with a leader list.  RANGE: a row outside
// [0, bank_rows) gathers zeros - the range first: an append outside it was dropped, so a pick that equals it names no row either.
template <bool RANGE>
__device__ __forceinline__ void rows_gather(const RowsAG &k, int g, const int *rows, const int *lead, int n_rows, int app, int b,
                                            int bank_rows)
{
    const int rl = k.row_len4[g];
    const usot_f32x4 *__restrict__ fresh = (const usot_f32x4 *)k.fresh[g] + (long)b * rl;
    const usot_f32x4 *__restrict__ bank = (const usot_f32x4 *)k.bank[g];
    usot_f32x4 *__restrict__ dst = (usot_f32x4 *)k.picked[g - 1] + (long)b * k.n_pick * rl;
    const int total = n_rows * rl;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / rl, e = i - r * rl;
        const int row = rows[lead ? lead[r] : r];
        usot_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!RANGE || (row >= 0 && row < bank_rows)) v = row == app ? fresh[e] : bank[(long)row * rl + e];
        dst[i] = v;
    }
}

// ---- SiamFC crop on the device (lib/utils/track_utils.py:30-119): window extraction with
// mean-colour padding, OpenCV-style fixed-point bilinear resize (the arithmetic restated in
// usot_amd/hostutils.py::resize_bilinear_u8) and HWC uint8 -> CHW float32, one output pixel per call.
struct CropK {
    const unsigned char *im;      // [H][W][3]
    float *out;                   // [3][S][S]
    int H, W, S, win;
    int x0, y0;                   // window origin in image coordinates (may be negative)
    int fill[3];
};

__device__ __forceinline__ void crop_axis(int d, int n_src, int n_dst, int &s0, int &s1, int &w0, int &w1)
{
    // OpenCV's own arithmetic (see hostutils._resize_axis): double scale = 1 / (dst / src), the source
    // coordinate rounded to float BEFORE the floor, float fraction, round-half-even coefficients
    const double scale = 1.0 / ((double)n_dst / (double)n_src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= n_src - 1) { f = 0.0f; s = n_src - 1; }
    w1 = (int)rintf(f * 2048.0f);
    w0 = (int)rintf((1.0f - f) * 2048.0f);
    s0 = s;
    s1 = min(s + 1, n_src - 1);
}

__device__ __forceinline__ int crop_px(const CropK &p, int wx, int wy, int c)
{
    const int ix = p.x0 + wx, iy = p.y0 + wy;
    if ((unsigned)ix >= (unsigned)p.W || (unsigned)iy >= (unsigned)p.H) return p.fill[c];
    return p.im[((long)iy * p.W + ix) * 3 + c];
}

// output pixel (dx, dy), all three channels
__device__ __forceinline__ void crop_resize_px(const CropK &p, int dx, int dy)
{
    if (p.win == p.S) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out[((long)c * p.S + dy) * p.S + dx] = (float)crop_px(p, dx, dy, c);
        return;
    }
    if (p.win == 2 * p.S) {          // exact 2x downscale: cv2.resize switches INTER_LINEAR to INTER_AREA
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = (crop_px(p, 2 * dx, 2 * dy, c) + crop_px(p, 2 * dx + 1, 2 * dy, c) +
                           crop_px(p, 2 * dx, 2 * dy + 1, c) + crop_px(p, 2 * dx + 1, 2 * dy + 1, c) + 2) >> 2;
            p.out[((long)c * p.S + dy) * p.S + dx] = (float)v;
        }
        return;
    }
    int xa, xb, wxa, wxb, ya, yb, wya, wyb;
    crop_axis(dx, p.win, p.S, xa, xb, wxa, wxb);
    crop_axis(dy, p.win, p.S, ya, yb, wya, wyb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long top = (long)crop_px(p, xa, ya, c) * wxa + (long)crop_px(p, xb, ya, c) * wxb;
        const long bot = (long)crop_px(p, xa, yb, c) * wxa + (long)crop_px(p, xb, yb, c) * wxb;
        long v = ((((long)wya * (top >> 4)) >> 16) + (((long)wyb * (bot >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        p.out[((long)c * p.S + dy) * p.S + dx] = (float)v;
    }
}

}  // namespace usot_head
