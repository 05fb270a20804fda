// Fused SGD step: every tensor of an optimiser in one launch, behind a device-side loss guard (usot_hip.h states the arithmetic,
// the table and the contract).  Everything here is bandwidth: 20 bytes per element, p, g and buf read, p and buf written.
//
// The kernel reads a device-resident table - T records of usot_sgd_tensor, then a list of {tensor, chunk_in_tensor} - that the host
// builds (usot_sgd_table_fill) and uploads when it changes.  One workgroup of 256 threads handles one chunk of SGD_CHUNK elements
// and strides over the chunk list by the grid (at most SGD_GRID_CAP workgroups: the rule for memory-bound kernels).  The chunk entry
// and the record are the same for the whole workgroup, so every branch on them is uniform.  A thread moves SGD_CHUNK / 1024 f32x4
// of each operand and issues all its loads before the first store (p, g and buf may not be assumed distinct by the compiler).
//
// The arithmetic is written with explicit fmaf under `fp contract(off)`: four fused multiply-adds and one product per element, the
// same instructions on the 16-byte path, on its scalar tail and on the scalar path, so a tensor's result does not depend on which
// path it took or on where it sits in the table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string.h>
#include "usot_hip.h"
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// the table's pointers come out of memory, so the compiler takes them for generic addresses (flat_load / flat_store); they are device
// allocations: say so, and the accesses are global_load / global_store
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

constexpr int SGD_THREADS = 256;
constexpr int SGD_CHUNK = 4096;            // elements per chunk: four f32x4 per thread
constexpr int SGD_GRID_CAP = 2048;
constexpr int SGD_PER = SGD_CHUNK / 4 / SGD_THREADS;
constexpr int SGD_FLAGS = USOT_SGD_FIRST | USOT_SGD_NESTEROV | USOT_SGD_MAXIMIZE;
static_assert(SGD_CHUNK % (4 * SGD_THREADS) == 0, "a chunk is a whole number of f32x4 per thread");
static_assert(sizeof(usot_sgd_tensor) == 56 && sizeof(usot_sgd_tensor) % 8 == 0, "the chunk list follows the records, 8-byte aligned");

struct SgdChunk {
    int32_t tensor, chunk;
};

struct SgdK {
    const usot_sgd_tensor *rec;
    const SgdChunk *chunks;
    const float *guard;
    int32_t *counters;
    int n_chunks, zero;
};

struct SgdHyp {
    float lr, wd, mu, gs;
    bool first, nesterov, maximize, mom;
};

__device__ __forceinline__ void sgd_one(const SgdHyp &h, float p, float g, float b, float &p2, float &b2)
{
#pragma clang fp contract(off)
    const float d = fmaf(h.wd, p, h.maximize ? -g : g);
    float step = d;
    b2 = b;
    if (h.mom) {
        b2 = h.first ? d : fmaf(h.mu, b, h.gs * d);
        step = h.nesterov ? fmaf(h.mu, b2, d) : b2;
    }
    p2 = fmaf(-h.lr, step, p);
}

__device__ __forceinline__ void sgd_four(const SgdHyp &h, f32x4 p, f32x4 g, f32x4 b, f32x4 &p2, f32x4 &b2)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk, bk;
        sgd_one(h, p[k], g[k], b[k], pk, bk);
        p2[k] = pk;
        b2[k] = bk;
    }
}

__global__ __launch_bounds__(SGD_THREADS) void sgd_step_f32(const SgdK a)
{
    const int tid = threadIdx.x;
    bool skip = false;
    if (a.guard) {
        const float loss = *a.guard;
        skip = !(loss <= 1e4f) || loss == -INFINITY;       // NaN, +Inf, > 1e4 | -Inf: the reference's is_valid_number, negated
    }
    if (a.counters && blockIdx.x == 0 && tid == 0) a.counters[skip ? 1 : 0] = a.counters[skip ? 1 : 0] + 1;
    if (skip && !a.zero) return;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const SgdChunk ch = a.chunks[c];
        const usot_sgd_tensor r = a.rec[ch.tensor];
        const long base = (long)ch.chunk * SGD_CHUNK;
        const long left = r.n - base;
        const int len = left < SGD_CHUNK ? (int)left : SGD_CHUNK;
        SgdHyp h;
        h.lr = r.lr; h.wd = r.weight_decay; h.mu = r.momentum; h.gs = r.grad_scale;
        h.first = (r.flags & USOT_SGD_FIRST) != 0;
        h.nesterov = (r.flags & USOT_SGD_NESTEROV) != 0;
        h.maximize = (r.flags & USOT_SGD_MAXIMIZE) != 0;
        h.mom = r.momentum != 0.f;
        const bool read_b = h.mom && !h.first;
        gfloat *P = (gfloat *)(r.p + base), *G = (gfloat *)(r.g + base), *B = (gfloat *)(h.mom ? r.buf + base : nullptr);
        const bool vec = (((uintptr_t)r.p | (uintptr_t)r.g | (uintptr_t)(h.mom ? r.buf : nullptr)) & 15) == 0;
        const int nv = vec ? len >> 2 : 0;                 // f32x4 of this chunk; the rest is scalar
        if (vec) {
            gf32x4 *P4 = (gf32x4 *)P, *G4 = (gf32x4 *)G, *B4 = (gf32x4 *)B;
            if (skip) {
#pragma unroll
                for (int k = 0; k < SGD_PER; ++k)
                    if (tid + k * SGD_THREADS < nv) G4[tid + k * SGD_THREADS] = zero4;
            } else {
                f32x4 vp[SGD_PER], vg[SGD_PER], vb[SGD_PER];
#pragma unroll
                for (int k = 0; k < SGD_PER; ++k) {
                    const int i = tid + k * SGD_THREADS;
                    vp[k] = vg[k] = vb[k] = zero4;
                    if (i < nv) {
                        vp[k] = P4[i];
                        vg[k] = G4[i];
                        if (read_b) vb[k] = B4[i];
                    }
                }
#pragma unroll
                for (int k = 0; k < SGD_PER; ++k) {
                    const int i = tid + k * SGD_THREADS;
                    if (i < nv) {
                        f32x4 p2, b2;
                        sgd_four(h, vp[k], vg[k], vb[k], p2, b2);
                        P4[i] = p2;
                        if (h.mom) B4[i] = b2;
                        if (a.zero) G4[i] = zero4;
                    }
                }
            }
        }
        // the scalar path: the n % 4 tail of an aligned tensor (at most three elements, in its last chunk), or the whole chunk
        for (int i = nv * 4 + tid; i < len; i += SGD_THREADS) {
            if (!skip) {
                float p2, b2;
                sgd_one(h, P[i], G[i], read_b ? B[i] : 0.f, p2, b2);
                P[i] = p2;
                if (h.mom) B[i] = b2;
            }
            if (a.zero) G[i] = 0.f;
        }
    }
}

bool word_aligned(const void *q) { return ((uintptr_t)q & 3) == 0; }
bool rate_ok(float v) { return isfinite(v) && v >= 0.f; }

bool record_ok(const usot_sgd_tensor &r)
{
    if (!r.p || !r.g || r.n < 0) return false;
    if (!word_aligned(r.p) || !word_aligned(r.g) || !word_aligned(r.buf)) return false;
    if (!rate_ok(r.lr) || !rate_ok(r.weight_decay) || !rate_ok(r.momentum) || !isfinite(r.grad_scale)) return false;
    if (r.momentum != 0.f && !r.buf) return false;
    if (r.flags & ~SGD_FLAGS) return false;
    if ((r.flags & USOT_SGD_NESTEROV) && (r.momentum == 0.f || r.grad_scale != 1.f)) return false;
    return true;
}

int64_t chunks_of(int64_t n) { return n / SGD_CHUNK + (n % SGD_CHUNK != 0); }

}  // namespace

extern "C" int usot_sgd_chunk_elems(void) { return SGD_CHUNK; }
extern "C" int usot_sgd_grid_cap(void) { return SGD_GRID_CAP; }

extern "C" int64_t usot_sgd_table_bytes(const int64_t *n, int T, int64_t *n_chunks)
{
    if (!n || T < 1) return USOT_EINVAL;
    int64_t chunks = 0;
    for (int i = 0; i < T; ++i) {
        if (n[i] < 0) return USOT_EINVAL;
        chunks += chunks_of(n[i]);
        if (chunks > INT32_MAX) return USOT_EINVAL;
    }
    if (n_chunks) *n_chunks = chunks;
    return (int64_t)T * (int64_t)sizeof(usot_sgd_tensor) + chunks * (int64_t)sizeof(SgdChunk);
}

extern "C" int usot_sgd_table_fill(const usot_sgd_tensor *t, int T, void *image, int64_t bytes)
{
    if (!t || !image || T < 1) return USOT_EINVAL;
    int64_t chunks = 0;
    for (int i = 0; i < T; ++i) {
        if (!record_ok(t[i])) return USOT_EINVAL;
        chunks += chunks_of(t[i].n);
        if (chunks > INT32_MAX) return USOT_EINVAL;
    }
    if (bytes < (int64_t)T * (int64_t)sizeof(usot_sgd_tensor) + chunks * (int64_t)sizeof(SgdChunk)) return USOT_EINVAL;
    char *out = (char *)image;
    for (int i = 0; i < T; ++i) {
        usot_sgd_tensor r = t[i];
        r.reserved = 0;
        memcpy(out + (size_t)i * sizeof r, &r, sizeof r);
    }
    out += (size_t)T * sizeof(usot_sgd_tensor);
    for (int i = 0; i < T; ++i)
        for (int64_t c = 0, e = chunks_of(t[i].n); c < e; ++c) {
            const SgdChunk ch = {i, (int32_t)c};
            memcpy(out, &ch, sizeof ch);
            out += sizeof ch;
        }
    return USOT_OK;
}

extern "C" int usot_sgd_step_f32(void *stream, const usot_sgd_launch *d)
{
    if (!d || !d->table || ((uintptr_t)d->table & 7) || d->T < 1 || d->n_chunks < 0 || d->n_chunks > INT32_MAX) return USOT_EINVAL;
    if (((uintptr_t)d->guard | (uintptr_t)d->counters) & 3) return USOT_EINVAL;
    if (d->n_chunks == 0) return USOT_OK;
    SgdK a;
    a.rec = (const usot_sgd_tensor *)d->table;
    a.chunks = (const SgdChunk *)((const char *)d->table + (size_t)d->T * sizeof(usot_sgd_tensor));
    a.guard = d->guard;
    a.counters = d->counters;
    a.n_chunks = (int)d->n_chunks;
    a.zero = d->zero_grads != 0;
    const int grid = a.n_chunks < SGD_GRID_CAP ? a.n_chunks : SGD_GRID_CAP;
    hipLaunchKernelGGL(sgd_step_f32, dim3((unsigned)grid), dim3(SGD_THREADS), 0, (hipStream_t)stream, a);
    USOT_CHECK_LAUNCH();
    return USOT_OK;
}
