// Lock-step multi-video tracking: the three per-video kernels of a frame graph (crop, memory append + gather, decode) in
// batched form, so that ONE launch serves the B videos ("slots") of a step (engine.BatchSession).  Each slot reads its own
// record of the step's control block (usot_slot_rec, include/usot_hip.h), once per workgroup; workgroups never hand data
// to each other.  The kernels here only fetch the slot's words and offset its pointers: everything they compute is the
// single-frame kernels' own code (head_common.h), so each slot is bit-identical to the single-frame kernel run on its data.
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

__device__ __forceinline__ const usot_slot_rec *slot_rec(const unsigned char *ctl, int b)
{
    return (const usot_slot_rec *)(ctl + USOT_STEP_HDR_BYTES) + b;
}

// ---- decode: one workgroup per slot (blockIdx.x), decode_kernel with the slot's maps, target size and result row
__global__ __launch_bounds__(1024) void decode_batch_kernel(
    const float *__restrict__ cls, const float *__restrict__ cls_mem, const float *__restrict__ bbox,
    const double *__restrict__ window, double *__restrict__ out, int S, int instance_size, int stride,
    float ratio, double penalty_k, double window_influence, const unsigned char *__restrict__ ctl, float *__restrict__ roi_out)
{
    const int b = blockIdx.x;
    __shared__ double ctl_w[3];
    if (threadIdx.x < 3) {                     // the slot's target size and the step tag: one round trip
        const usot_slot_rec *rec = slot_rec(ctl, b);
        ctl_w[threadIdx.x] = threadIdx.x < 2 ? rec->tsz[threadIdx.x] : *(const double *)ctl;
    }
    __syncthreads();
    const double tw = ctl_w[0], th = ctl_w[1], tag = ctl_w[2];
    const int n = S * S;
    out += (long)b * 16;
    DecCell best;
    if (!dec_scan_argmax(best, cls + (long)b * n, cls_mem + (long)b * n, bbox + (long)b * 4 * n, window, S, instance_size, stride,
                         ratio, penalty_k, window_influence, tw, th))
        return;
    dec_publish(best, out, roi_out + (long)b * 5, (float)b, S, instance_size, stride);
    // results first, system-scope fence, then this slot's tag (the host polls all B tags)
    __threadfence_system();
    out[8] = tag;
}

// ---- append + gather: blockIdx.z = slot, rows_append_gather_kernel per slot with the slot record's picks and append row.
// Rows outside [0, bank_rows = k.arg) are never touched: such an append is dropped, such a pick gathers zeros.
__global__ __launch_bounds__(256) void rows_append_gather_batch_kernel(const RowsAG k, const unsigned char *__restrict__ ctl)
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
    if (job >= 4) rows_gather<true>(k, job - 3, rows, nullptr, k.n_pick, app, b, k.arg);
    else if (app >= 0 && app < k.arg) rows_append_row(k, job, app, b);
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
    RowsAG k;
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
    k.n_pick = n_pick; k.arg = bank_rows;
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
