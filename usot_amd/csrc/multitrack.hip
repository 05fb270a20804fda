// Lock-step multi-video tracking: the three per-video kernels of a frame graph (crop, memory append + gather, decode) in
// batched form, so that ONE launch serves the B videos ("slots") of a step (engine.BatchSession).  Each slot reads its own
// record of the step's control block (usot_slot_rec, include/usot_hip.h), once per workgroup; workgroups never hand data
// to each other.  The per-element arithmetic is the single-frame kernels' own (head_common.h, and the decode's per-cell
// expressions below, restated from head_ops.hip's decode_kernel in the same order): each slot is bit-identical to the
// single-frame kernel run on that slot's data.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "usot_hip.h"
#include "common.h"
#include "head_common.h"

static_assert(sizeof(usot_slot_rec) == 192, "usot_slot_rec layout");
static_assert(offsetof(usot_slot_rec, im) == 16 && offsetof(usot_slot_rec, append_row) == 56 &&
              offsetof(usot_slot_rec, picks) == 64, "usot_slot_rec layout");

namespace {

using namespace usot_head;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const usot_slot_rec *slot_rec(const unsigned char *ctl, int b)
{
    return (const usot_slot_rec *)(ctl + USOT_STEP_HDR_BYTES) + b;
}

// ---- decode: one workgroup per slot (blockIdx.x), decode_kernel's body with the slot's maps, target size and row
__global__ __launch_bounds__(1024) void decode_batch_kernel(
    const float *__restrict__ cls, const float *__restrict__ cls_mem, const float *__restrict__ bbox,
    const double *__restrict__ window, double *__restrict__ out, int S, int instance_size, int stride,
    float ratio, double penalty_k, double window_influence, const unsigned char *__restrict__ ctl, float *__restrict__ roi_out)
{
    const int b = blockIdx.x;
    __shared__ double ctl_w[3];
    __shared__ double wave_v[16];
    __shared__ int wave_i[16];
    __shared__ int win_i;
    if (threadIdx.x < 3) {                     // the slot's target size and the step tag: one round trip
        const usot_slot_rec *rec = slot_rec(ctl, b);
        ctl_w[threadIdx.x] = threadIdx.x < 2 ? rec->tsz[threadIdx.x] : *(const double *)ctl;
    }
    __syncthreads();
    const double tw = ctl_w[0], th = ctl_w[1], tag = ctl_w[2];
    const int n = S * S;
    cls += (long)b * n;
    cls_mem += (long)b * n;
    bbox += (long)b * 4 * n;
    out += (long)b * 16;
    const double tpad = (tw + th) * 0.5;
    const double tsz = sqrt((tw + tpad) * (th + tpad));
    const double tratio = tw / th;
    DecCell best;
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
    if (best.i == win_i) {
        out[0] = (double)best.i;
        out[1] = (double)best.sc;
        out[2] = best.pen;
        out[3] = best.x1; out[4] = best.y1; out[5] = best.x2; out[6] = best.y2;
        out[7] = best.ps;
        // pool_label_search (usot_tracker.py:329-350), as decode_kernel; batch index = the slot
        const double lo = (double)((0 - S / 2) * stride + instance_size / 2);
        const double hi = (double)((S - 1 - S / 2) * stride + instance_size / 2);
        const double slope = (double)(2 * (S / 2)) / (hi - lo);
        const double gap = 1.0 / slope;
        const double bx[4] = {best.x1, best.y1, best.x2, best.y2};
        float *roi = roi_out + (long)b * 5;
        roi[0] = (float)b;
        for (int e = 0; e < 4; ++e) {
            double v = (double)(float)bx[e];
            v = v < lo - gap ? lo - gap : (v > hi + gap ? hi + gap : v);      // np.clip: a NaN stays a NaN (fmax / fmin would drop it)
            roi[1 + e] = (float)((v - lo) * slope);
        }
        // results first, system-scope fence, then this slot's tag (the host polls all B tags)
        __threadfence_system();
        out[8] = tag;
    }
}

// ---- append + gather: blockIdx.z = slot, blockIdx.y: 0-3 = append bank y, 4-6 = gather bank y - 3 (rows_append_gather_kernel
// per slot).  Rows outside [0, bank_rows) are never touched: such an append is dropped, such a pick gathers zeros.
struct RowsAGB {
    const float *fresh[4];
    float *bank[4];
    float *picked[3];
    int row_len4[4];
    int n_pick, bank_rows;
};

__global__ __launch_bounds__(256) void rows_append_gather_batch_kernel(const RowsAGB k, const unsigned char *__restrict__ ctl)
{
    const int b = blockIdx.z;
    __shared__ int rows[33];
    {
        const usot_slot_rec *rec = slot_rec(ctl, b);
        if (threadIdx.x < k.n_pick) rows[threadIdx.x] = rec->picks[threadIdx.x];
        if (threadIdx.x == 32) rows[32] = rec->append_row;
    }
    __syncthreads();
    const int app = rows[32];
    const int job = blockIdx.y;
    if (job < 4) {
        if (app < 0 || app >= k.bank_rows) return;
        const int rl = k.row_len4[job];
        const f32x4 *__restrict__ src = (const f32x4 *)k.fresh[job] + (long)b * rl;
        f32x4 *__restrict__ dst = (f32x4 *)k.bank[job] + (long)app * rl;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < rl; i += gridDim.x * 256) dst[i] = src[i];
        return;
    }
    const int g = job - 3;
    const int rl = k.row_len4[g];
    const f32x4 *__restrict__ fresh = (const f32x4 *)k.fresh[g] + (long)b * rl;
    const f32x4 *__restrict__ bank = (const f32x4 *)k.bank[g];
    f32x4 *__restrict__ dst = (f32x4 *)k.picked[g - 1] + (long)b * k.n_pick * rl;
    const int total = k.n_pick * rl;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / rl, e = i - r * rl;
        const int row = rows[r];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        // the range first: an append outside it was dropped, so a pick that equals it names no row either
        if (row >= 0 && row < k.bank_rows) v = row == app ? fresh[e] : bank[(long)row * rl + e];
        dst[i] = v;
    }
}

// ---- crop + resize: blockIdx.y = slot, a grid-stride loop over its S x S output pixels
__global__ __launch_bounds__(256) void crop_resize_batch_kernel(const unsigned char *__restrict__ ctl, float *__restrict__ out, int S)
{
    const int b = blockIdx.y;
    __shared__ int w[10];         // usot_slot_rec int32 words 4 .. 13: im (lo, hi), H, W, x0, y0, win, fill[3]
    if (threadIdx.x < 10) w[threadIdx.x] = ((const int32_t *)slot_rec(ctl, b))[4 + threadIdx.x];
    __syncthreads();
    const uint64_t im = (uint64_t)(uint32_t)w[0] | ((uint64_t)(uint32_t)w[1] << 32);
    if (!im || w[2] <= 0 || w[3] <= 0 || w[6] <= 0) return;
    const CropK p{(const unsigned char *)(uintptr_t)im, out + (long)b * 3 * S * S, w[2], w[3], S, w[6], w[4], w[5], {w[7], w[8], w[9]}};
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < S * S; idx += gridDim.x * 256) {
        const int dy = idx / S, dx = idx - dy * S;
        crop_resize_px(p, dx, dy);
    }
}

// one thread per response cell up to 1024 cells (S <= 32), whole wavefronts (head_ops.hip: decode_threads)
inline unsigned decode_threads(int S)
{
    const int n = S * S;
    return (unsigned)(n >= 1024 ? 1024 : (n + 63) / 64 * 64);
}

}  // namespace

extern "C" int usot_decode_batch_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox, const double *window,
                                     double *out, int B, int S, int instance_size, int stride, float ratio, double penalty_k,
                                     double window_influence, const void *ctl, float *roi_out)
{
    if (!cls || !cls_mem || !bbox || !window || !out || !ctl || !roi_out || B < 1 || B > 65535 || S < 1 || S > 32)
        return USOT_EINVAL;
    hipLaunchKernelGGL(decode_batch_kernel, dim3(B), dim3(decode_threads(S)), 0, (hipStream_t)stream, cls, cls_mem, bbox,
                       window, out, S, instance_size, stride, ratio, penalty_k, window_influence, (const unsigned char *)ctl, roi_out);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_rows_append_gather_batch_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                                 const int32_t *row_len, const void *ctl, int B, int n_pick, int bank_rows)
{
    if (!fresh || !bank || !picked || !row_len || !ctl || B < 1 || B > 65535 || n_pick < 1 || n_pick > 32 || bank_rows < 1)
        return USOT_EINVAL;
    RowsAGB k;
    long most = 0;
    for (int i = 0; i < 4; ++i) {
        if (!fresh[i] || !bank[i] || row_len[i] <= 0 || (row_len[i] & 3)) return USOT_EINVAL;
        if (((uintptr_t)fresh[i] % 16) || ((uintptr_t)bank[i] % 16)) return USOT_EINVAL;
        if (i && (!picked[i - 1] || ((uintptr_t)picked[i - 1] % 16))) return USOT_EINVAL;
        k.fresh[i] = fresh[i]; k.bank[i] = bank[i]; k.row_len4[i] = row_len[i] / 4;
        if (i) k.picked[i - 1] = picked[i - 1];
        const long t = (long)(i ? n_pick : 1) * k.row_len4[i];
        if (t > most) most = t;
    }
    if (most > 0x3fffffffL || (long)bank_rows * k.row_len4[0] > (1L << 40)) return USOT_EINVAL;
    k.n_pick = n_pick; k.bank_rows = bank_rows;
    const int blocks = (int)((most + 255) / 256 > 64 ? 64 : (most + 255) / 256);
    hipLaunchKernelGGL(rows_append_gather_batch_kernel, dim3(blocks, 7, B), dim3(256), 0, (hipStream_t)stream, k,
                       (const unsigned char *)ctl);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}

extern "C" int usot_crop_resize_batch_u8_f32(void *stream, const void *ctl, float *out, int B, int S)
{
    if (!ctl || !out || B < 1 || B > 65535 || S < 1 || S > 4096) return USOT_EINVAL;
    const int blocks = usot_cdiv((long)S * S, 256) > 128 ? 128 : usot_cdiv((long)S * S, 256);
    hipLaunchKernelGGL(crop_resize_batch_kernel, dim3(blocks, B), dim3(256), 0, (hipStream_t)stream, (const unsigned char *)ctl, out, S);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}
