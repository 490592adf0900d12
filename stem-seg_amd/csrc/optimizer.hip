// The optimiser step of training (the reference's training/utils.py:195-210: torch.optim.SGD with momentum / Nesterov / weight decay, or
// torch.optim.Adam), the global gradient norm and the clip coefficient of torch.nn.utils.clip_grad_norm_: one launch over every tensor of a
// parameter group instead of several foreach passes.
//
//   tables (include/stemseg_hip.h): a device array of StemsegOptTensor descriptors { p, g, state1, state2, n, flags } and a device array of
//     StemsegOptChunk { tensor, chunk } pairs, chunk k of a tensor being its elements [k * STEMSEG_OPT_CHUNK, min(n, (k + 1) * STEMSEG_OPT_CHUNK)).
//     A chunk never straddles tensors, so the chunk table is a function of the tensor sizes alone (stemseg_hip_opt_plan builds it on the
//     host and checks the descriptors); hyper-parameters travel by value, so a new learning rate needs no new table.
//   launch: min(chunks, kMaxWg) workgroups of 256 threads stride over the chunk table.  A chunk starts at a multiple of 16 bytes from its
//     tensor's base, so where the bases of p, g and the states in use are 16-byte aligned the body of a chunk goes through float4 loads and
//     stores and only the ragged tail (n % 4 elements of the last chunk) through scalars; otherwise the whole chunk does.  Both paths run
//     the same fp32 operations per element, so the bits do not depend on the path.  Nothing is written at or past element n.
//   arithmetic: torch's _single_tensor_sgd / _single_tensor_adam on the CPU, operation by operation in fp32 -- an `add(x, alpha = a)` there is
//     one fused multiply-add, `lerp_` is fma(w, g - m, m), `addcmul_` is fma(value * g, g, v), `addcdiv_` is p + (value * m) / denom -- with
//     contraction switched off everywhere else, so the device rounds where torch rounds.  g is read, never written.
//   gradient norm (2 launches): per chunk the fp64 sum of the squares (an fp32 square is exact in fp64) in a fixed tree order and a flag for a
//     non-finite element; then one workgroup adds the chunks' sums, each thread a run of consecutive chunks and the runs in a fixed tree, and
//     writes the norm (fp64), the OR of the flags (int32) and coef = min(1, max_norm / (norm + 1e-6)) (fp32) to device scalars.  The step
//     kernels take a pointer to such a scalar and multiply every gradient element by it first: a clip costs no read-back and no pass over g.
//   gradient bucket (data-parallel training): stemseg_hip_opt_bucket_plan lays the tensors of a table end to end in one flat fp32 buffer, each
//     slice rounded up to 4 elements so that every slice of a 16-byte-aligned bucket is 16-byte aligned; pack_grads copies (scale 1: the bits)
//     or scales every gradient into its slice over the same chunk table, zeros for a tensor without a gradient and for the padding;
//     unpack_grads copies slices back out; reduce_ranks turns the [world][total] result of an all-gather into the mean, summed in fp64 in
//     rising rank order and rounded once, so the result does not depend on a backend's summation order.  A kernel skips a slice that does
//     not lie inside [0, total): a damaged offset table addresses nothing.
// No floating-point atomics: two runs give identical bits.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace stemseg {
namespace {

constexpr int kOT = 256;                       // threads per workgroup
constexpr int kMaxWg = 2048;                   // grid cap: 256 CUs x 8 workgroups, the rest is strode over
constexpr int kChunk = STEMSEG_OPT_CHUNK;
static_assert(kChunk % (4 * kOT) == 0, "a chunk is a whole number of float4 rounds of a workgroup");

struct Hyper {
    float lr, mu, omd, wd;                     // SGD: learning rate, momentum, 1 - dampening, weight decay
    float omb1, b2, omb2, eps;                 // Adam: 1 - beta1, beta2, 1 - beta2, eps
    int nesterov;
};

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// one element of torch's _single_tensor_sgd; kMom: a momentum buffer exists (mu != 0)
template <bool kMom>
__device__ __forceinline__ void sgd_elem(const Hyper& h, bool scaled, float s, bool first, float& p, float g, float& buf) {
#pragma clang fp contract(off)
    if (scaled) g = g * s;
    if (h.wd != 0.f) g = fmaf(h.wd, p, g);
    if (kMom) {
        if (first) {
            buf = g;
        } else {
            buf = buf * h.mu;
            buf = fmaf(h.omd, g, buf);
        }
        g = h.nesterov ? fmaf(h.mu, buf, g) : buf;
    }
    p = fmaf(-h.lr, g, p);
}

// one element of torch's _single_tensor_adam (L2 weight decay, no amsgrad); neg_step = -(lr / bias_correction1), bc2s = sqrt(bias_correction2)
__device__ __forceinline__ void adam_elem(const Hyper& h, bool scaled, float s, float neg_step, float bc2s, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    if (scaled) g = g * s;
    if (h.wd != 0.f) g = fmaf(h.wd, p, g);
    m = fmaf(h.omb1, g - m, m);
    v = v * h.b2;
    v = fmaf(h.omb2 * g, g, v);
    const float denom = sqrtf(v) / bc2s + h.eps;
    p = p + (neg_step * m) / denom;
}

// the extent of chunk `c` of the table, or false for an entry that does not lie inside its tensor (never true for a table from
// stemseg_hip_opt_plan: the check keeps a damaged table from addressing anything)
__device__ __forceinline__ bool chunk_extent(const StemsegOptTensor* __restrict__ desc, int n_tensors, const StemsegOptChunk* __restrict__ chunks,
                                             long long c, StemsegOptTensor* d, long long* base, int* len) {
    const StemsegOptChunk r = chunks[c];
    if (r.tensor < 0 || r.tensor >= n_tensors || r.chunk < 0) return false;
    *d = desc[r.tensor];
    *base = (long long)r.chunk * kChunk;
    if (*base >= d->n) return false;
    *len = d->n - *base < kChunk ? (int)(d->n - *base) : kChunk;
    return true;
}

template <bool kMom>
__global__ __launch_bounds__(kOT) void sgd_step_kernel(const StemsegOptTensor* __restrict__ desc, int n_tensors,
                                                       const StemsegOptChunk* __restrict__ chunks, long long n_chunks, Hyper h,
                                                       const float* __restrict__ scale) {
    const bool scaled = scale != nullptr;
    const float s = scaled ? *scale : 1.f;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        StemsegOptTensor d;
        long long base;
        int len;
        if (!chunk_extent(desc, n_tensors, chunks, c, &d, &base, &len)) continue;
        const bool first = (d.flags & STEMSEG_OPT_STATE_UNINIT) != 0;
        float* p = d.p + base;
        const float* g = d.g + base;
        float* b = kMom ? d.state1 + base : nullptr;
        const int nvec = aligned16(d.p, d.g, kMom ? d.state1 : nullptr, nullptr) ? len / 4 : 0;
        for (int i = threadIdx.x; i < nvec; i += kOT) {
            float4 pv = reinterpret_cast<float4*>(p)[i];
            const float4 gv = reinterpret_cast<const float4*>(g)[i];
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kMom && !first) bv = reinterpret_cast<float4*>(b)[i];
            sgd_elem<kMom>(h, scaled, s, first, pv.x, gv.x, bv.x);
            sgd_elem<kMom>(h, scaled, s, first, pv.y, gv.y, bv.y);
            sgd_elem<kMom>(h, scaled, s, first, pv.z, gv.z, bv.z);
            sgd_elem<kMom>(h, scaled, s, first, pv.w, gv.w, bv.w);
            reinterpret_cast<float4*>(p)[i] = pv;
            if (kMom) reinterpret_cast<float4*>(b)[i] = bv;
        }
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) {
            float pv = p[i], bv = (kMom && !first) ? b[i] : 0.f;
            sgd_elem<kMom>(h, scaled, s, first, pv, g[i], bv);
            p[i] = pv;
            if (kMom) b[i] = bv;
        }
    }
}

__global__ __launch_bounds__(kOT) void adam_step_kernel(const StemsegOptTensor* __restrict__ desc, int n_tensors,
                                                        const StemsegOptChunk* __restrict__ chunks, long long n_chunks, Hyper h,
                                                        const float* __restrict__ scalars, const float* __restrict__ scale) {
    const bool scaled = scale != nullptr;
    const float s = scaled ? *scale : 1.f;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        StemsegOptTensor d;
        long long base;
        int len;
        if (!chunk_extent(desc, n_tensors, chunks, c, &d, &base, &len)) continue;
        const int ti = chunks[c].tensor;
        const float neg_step = -scalars[2 * ti], bc2s = scalars[2 * ti + 1];
        float* p = d.p + base;
        const float* g = d.g + base;
        float* m = d.state1 + base;
        float* v = d.state2 + base;
        const int nvec = aligned16(d.p, d.g, d.state1, d.state2) ? len / 4 : 0;
        for (int i = threadIdx.x; i < nvec; i += kOT) {
            float4 pv = reinterpret_cast<float4*>(p)[i];
            const float4 gv = reinterpret_cast<const float4*>(g)[i];
            float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            adam_elem(h, scaled, s, neg_step, bc2s, pv.x, gv.x, mv.x, vv.x);
            adam_elem(h, scaled, s, neg_step, bc2s, pv.y, gv.y, mv.y, vv.y);
            adam_elem(h, scaled, s, neg_step, bc2s, pv.z, gv.z, mv.z, vv.z);
            adam_elem(h, scaled, s, neg_step, bc2s, pv.w, gv.w, mv.w, vv.w);
            reinterpret_cast<float4*>(p)[i] = pv;
            reinterpret_cast<float4*>(m)[i] = mv;
            reinterpret_cast<float4*>(v)[i] = vv;
        }
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) {
            float pv = p[i], mv = m[i], vv = v[i];
            adam_elem(h, scaled, s, neg_step, bc2s, pv, g[i], mv, vv);
            p[i] = pv;
            m[i] = mv;
            v[i] = vv;
        }
    }
}

// ------------------------------------------------------------------------------------------------ gradient norm
// sum over the workgroup in a fixed tree order; thread 0 holds the result
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int off = kOT / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ void square_in(float x, double& acc, int& bad) {
    acc += (double)x * (double)x;
    bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(kOT) void grad_sq_partial_kernel(const StemsegOptTensor* __restrict__ desc, int n_tensors,
                                                              const StemsegOptChunk* __restrict__ chunks, long long n_chunks,
                                                              double* __restrict__ part, int* __restrict__ part_flag) {
    __shared__ double sh[kOT];
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        StemsegOptTensor d;
        long long base;
        int len;
        double acc = 0.0;
        int bad = 0;
        if (chunk_extent(desc, n_tensors, chunks, c, &d, &base, &len)) {
            const float* g = d.g + base;
            const int nvec = aligned16(d.g, nullptr, nullptr, nullptr) ? len / 4 : 0;
            for (int i = threadIdx.x; i < nvec; i += kOT) {
                const float4 gv = reinterpret_cast<const float4*>(g)[i];
                square_in(gv.x, acc, bad);
                square_in(gv.y, acc, bad);
                square_in(gv.z, acc, bad);
                square_in(gv.w, acc, bad);
            }
            for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) square_in(g[i], acc, bad);
        }
        const double sum = block_sum(acc, sh);
        const int any = __syncthreads_or(bad);
        if (threadIdx.x == 0) {
            part[c] = sum;
            part_flag[c] = any ? 1 : 0;
        }
    }
}

// max_norm < 0: no clip asked for, coef = 1
__global__ __launch_bounds__(kOT) void grad_norm_final_kernel(const double* __restrict__ part, const int* __restrict__ part_flag, long long n_chunks,
                                                              double max_norm, double* __restrict__ norm, float* __restrict__ coef,
                                                              int* __restrict__ flag) {
    __shared__ double sh[kOT];
    const long long per = (n_chunks + kOT - 1) / kOT, lo = threadIdx.x * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    double acc = 0.0;
    int bad = 0;
    for (long long c = lo; c < hi; ++c) {
        acc += part[c];
        bad |= part_flag[c];
    }
    const double sum = block_sum(acc, sh);
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(sum);
        *norm = nrm;
        *flag = any ? 1 : 0;
        double k = 1.0;
        if (max_norm >= 0.0) {
            k = max_norm / (nrm + 1e-6);
            k = k > 1.0 ? 1.0 : k;                 // (a NaN norm gives a NaN coefficient, as torch.clamp does)
        }
        *coef = (float)k;
    }
}

// ------------------------------------------------------------------------------------------------ gradient bucket
// the slice of tensor `t` in a bucket of `total` elements, or false where the offset table does not keep it inside the bucket
__device__ __forceinline__ bool slice_offset(const long long* __restrict__ offsets, int t, long long n, long long total, long long* off) {
    const long long o = offsets[t], padded = (n + 3) & ~3ll;
    if (o < 0 || (o & 3) != 0 || padded > total || o > total - padded) return false;
    *off = o;
    return true;
}

// bucket[offset[t] + i] = g_t[i] * scale (kCopy: the bits of g_t[i]); +0.0f for a tensor without a gradient and for the padding behind a slice.
// The bucket side of a chunk is always 16-byte aligned; a gradient that is the bucket slice itself (accumulated in place) is scaled in place.
template <bool kCopy>
__global__ __launch_bounds__(kOT) void pack_grads_kernel(const StemsegOptTensor* __restrict__ desc, int n_tensors,
                                                         const StemsegOptChunk* __restrict__ chunks, long long n_chunks,
                                                         const long long* __restrict__ offsets, float* bucket, long long total, float scale) {
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        StemsegOptTensor d;
        long long base, off;
        int len;
        if (!chunk_extent(desc, n_tensors, chunks, c, &d, &base, &len)) continue;
        if (!slice_offset(offsets, chunks[c].tensor, d.n, total, &off)) continue;
        float* dst = bucket + off + base;
        const float* g = d.g != nullptr ? d.g + base : nullptr;
        const int nvec = (g == nullptr || aligned16(d.g, nullptr, nullptr, nullptr)) ? len / 4 : 0;
        for (int i = threadIdx.x; i < nvec; i += kOT) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g != nullptr) {
                v = reinterpret_cast<const float4*>(g)[i];
                if (!kCopy) {
                    v.x = v.x * scale;
                    v.y = v.y * scale;
                    v.z = v.z * scale;
                    v.w = v.w * scale;
                }
            }
            reinterpret_cast<float4*>(dst)[i] = v;
        }
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) dst[i] = g == nullptr ? 0.f : (kCopy ? g[i] : g[i] * scale);
        if (base + len == d.n) {                   // the tensor's last chunk: the padding up to the next multiple of 4
            const int end = (len + 3) & ~3;
            for (int i = len + threadIdx.x; i < end; i += kOT) dst[i] = 0.f;
        }
    }
}

// p_t[i] = bucket[offset[t] + i]; a NULL p is skipped
__global__ __launch_bounds__(kOT) void unpack_grads_kernel(const StemsegOptTensor* __restrict__ desc, int n_tensors,
                                                           const StemsegOptChunk* __restrict__ chunks, long long n_chunks,
                                                           const long long* __restrict__ offsets, const float* bucket, long long total) {
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        StemsegOptTensor d;
        long long base, off;
        int len;
        if (!chunk_extent(desc, n_tensors, chunks, c, &d, &base, &len)) continue;
        if (d.p == nullptr || !slice_offset(offsets, chunks[c].tensor, d.n, total, &off)) continue;
        const float* src = bucket + off + base;
        float* p = d.p + base;
        const int nvec = aligned16(d.p, nullptr, nullptr, nullptr) ? len / 4 : 0;
        for (int i = threadIdx.x; i < nvec; i += kOT) reinterpret_cast<float4*>(p)[i] = reinterpret_cast<const float4*>(src)[i];
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) p[i] = src[i];
    }
}

// bucket[i] = float((double(gathered[0][i]) + double(gathered[1][i]) + ...) / double(world)): fp64 additions in rising rank order, one
// rounding to fp32.  vec: gathered, bucket and every row of gathered are 16-byte aligned
__global__ __launch_bounds__(kOT) void reduce_ranks_kernel(const float* __restrict__ gathered, int world, long long total, float* __restrict__ bucket,
                                                           long long n_chunks, int vec) {
    const double w = (double)world;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long base = c * kChunk;
        const int len = total - base < kChunk ? (int)(total - base) : kChunk;
        const float* src = gathered + base;
        float* dst = bucket + base;
        const int nvec = vec ? len / 4 : 0;
        for (int i = threadIdx.x; i < nvec; i += kOT) {
            const float4 v0 = reinterpret_cast<const float4*>(src)[i];
            double a = v0.x, b = v0.y, e = v0.z, f = v0.w;
            for (int r = 1; r < world; ++r) {
                const float4 v = reinterpret_cast<const float4*>(src + (long long)r * total)[i];
                a += (double)v.x;
                b += (double)v.y;
                e += (double)v.z;
                f += (double)v.w;
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4((float)(a / w), (float)(b / w), (float)(e / w), (float)(f / w));
        }
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kOT) {
            double a = src[i];
            for (int r = 1; r < world; ++r) a += (double)src[(long long)r * total + i];
            dst[i] = (float)(a / w);
        }
    }
}

int check_tables(const char* who, const void* desc, int32_t n_tensors, const void* chunks, int64_t n_chunks) {
    SS_CHECK_ARG(desc != nullptr && chunks != nullptr, "%s: null table", who);
    SS_CHECK_ARG(n_tensors > 0, "%s: n_tensors %d must be positive", who, n_tensors);
    SS_CHECK_ARG(n_chunks > 0 && n_chunks < (1ll << 31), "%s: n_chunks %lld outside 1..2^31 - 1", who, (long long)n_chunks);
    SS_CHECK_ARG(((uintptr_t)desc & 7) == 0 && ((uintptr_t)chunks & 7) == 0, "%s: the tables must be 8-byte aligned", who);
    return STEMSEG_OK;
}

int make_hyper(const char* who, const StemsegOptHyper* hy, Hyper* h) {
    SS_CHECK_ARG(hy != nullptr, "%s: null hyper-parameters", who);
    SS_CHECK_ARG(hy->struct_bytes == (int32_t)sizeof(StemsegOptHyper), "%s: hyper-parameter struct size mismatch (%d vs %d): ABI skew", who,
                 hy->struct_bytes, (int)sizeof(StemsegOptHyper));
    SS_CHECK_ARG((hy->flags & ~STEMSEG_OPT_NESTEROV) == 0, "%s: unknown flag in 0x%x", who, (unsigned)hy->flags);
    h->lr = hy->lr;
    h->mu = hy->momentum;
    h->omd = hy->one_minus_dampening;
    h->wd = hy->weight_decay;
    h->omb1 = hy->one_minus_beta1;
    h->b2 = hy->beta2;
    h->omb2 = hy->one_minus_beta2;
    h->eps = hy->eps;
    h->nesterov = (hy->flags & STEMSEG_OPT_NESTEROV) ? 1 : 0;
    return STEMSEG_OK;
}

// what the bucket entry points share: the tables, the offsets, the bucket and a total that the chunk count allows.  The descriptors live in
// device memory, so the host sees the sizes only through n_tensors and n_chunks: a tensor of k chunks holds more than (k - 1) and at most k
// chunks' worth of elements, which bounds the plan's total from both sides; the kernels hold every slice to [0, total) themselves.
int check_bucket(const char* who, const void* desc, int32_t n_tensors, const void* chunks, int64_t n_chunks, const void* offsets, const void* bucket,
                 int64_t total) {
    if (int rc = check_tables(who, desc, n_tensors, chunks, n_chunks)) return rc;
    SS_CHECK_ARG(offsets != nullptr && bucket != nullptr, "%s: null offsets or bucket", who);
    SS_CHECK_ARG(((uintptr_t)offsets & 7) == 0, "%s: the offsets must be 8-byte aligned", who);
    SS_CHECK_ARG(((uintptr_t)bucket & 15) == 0, "%s: the bucket must be 16-byte aligned", who);
    SS_CHECK_ARG(total > 0 && total % 4 == 0, "%s: total %lld is not a positive multiple of 4, which stemseg_hip_opt_bucket_plan's always is", who,
                 (long long)total);
    SS_CHECK_ARG(total <= n_chunks * (int64_t)kChunk && total > (n_chunks - n_tensors) * (int64_t)kChunk,
                 "%s: total %lld is not the plan's: %lld chunks over %d tensors hold more than %lld and at most %lld elements", who, (long long)total,
                 (long long)n_chunks, n_tensors, (long long)((n_chunks - n_tensors) * (int64_t)kChunk), (long long)(n_chunks * (int64_t)kChunk));
    return STEMSEG_OK;
}

}  // namespace
}  // namespace stemseg

using namespace stemseg;

extern "C" int stemseg_hip_opt_plan(const StemsegOptTensor* tensors_host, int32_t n_tensors, int32_t n_states, StemsegOptChunk* chunks_host,
                                    int64_t chunks_cap, int64_t* n_chunks) {
    SS_CHECK_ARG(tensors_host != nullptr && n_chunks != nullptr, "opt_plan: null pointer");
    SS_CHECK_ARG(n_tensors > 0, "opt_plan: n_tensors %d must be positive", n_tensors);
    SS_CHECK_ARG(n_states >= 0 && n_states <= 2, "opt_plan: n_states %d outside 0..2", n_states);
    int64_t total = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const StemsegOptTensor& d = tensors_host[t];
        SS_CHECK_ARG(d.n >= 0, "opt_plan: tensor %d has a negative element count %lld", t, (long long)d.n);
        SS_CHECK_ARG((d.flags & ~STEMSEG_OPT_STATE_UNINIT) == 0 && d.reserved == 0, "opt_plan: tensor %d has an unknown flag in 0x%x", t,
                     (unsigned)d.flags);
        SS_CHECK_ARG(d.n == 0 || (d.p != nullptr && d.g != nullptr), "opt_plan: tensor %d has a null p or g", t);
        SS_CHECK_ARG(d.n == 0 || ((n_states < 1 || d.state1 != nullptr) && (n_states < 2 || d.state2 != nullptr)),
                     "opt_plan: tensor %d lacks a state buffer (%d asked for)", t, n_states);
        SS_CHECK_ARG((((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.state1 | (uintptr_t)d.state2) & 3) == 0,
                     "opt_plan: tensor %d has a pointer that is not 4-byte aligned", t);
        const int64_t k = ceil_div(d.n, (int64_t)STEMSEG_OPT_CHUNK);
        SS_CHECK_ARG(k < (1ll << 31) && total + k < (1ll << 31), "opt_plan: more than 2^31 - 1 chunks");
        if (chunks_host != nullptr) {
            SS_CHECK_ARG(total + k <= chunks_cap, "opt_plan: the chunk table holds %lld entries, more are needed", (long long)chunks_cap);
            for (int64_t c = 0; c < k; ++c) {
                chunks_host[total + c].tensor = t;
                chunks_host[total + c].chunk = (int32_t)c;
            }
        }
        total += k;
    }
    *n_chunks = total;
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_sgd_step(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                        const StemsegOptHyper* hyper, const float* grad_scale, void* stream) {
    if (int rc = check_tables("opt_sgd_step", tensors, n_tensors, chunks, n_chunks)) return rc;
    Hyper h;
    if (int rc = make_hyper("opt_sgd_step", hyper, &h)) return rc;
    SS_CHECK_ARG(((uintptr_t)grad_scale & 3) == 0, "opt_sgd_step: grad_scale must be 4-byte aligned");
    const dim3 grid((unsigned)std::min<int64_t>(n_chunks, kMaxWg));
    if (h.mu != 0.f)
        hipLaunchKernelGGL(sgd_step_kernel<true>, grid, dim3(kOT), 0, as_stream(stream), tensors, n_tensors, chunks, (long long)n_chunks, h, grad_scale);
    else
        hipLaunchKernelGGL(sgd_step_kernel<false>, grid, dim3(kOT), 0, as_stream(stream), tensors, n_tensors, chunks, (long long)n_chunks, h, grad_scale);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_adam_step(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                         const StemsegOptHyper* hyper, const float* tensor_scalars, const float* grad_scale, void* stream) {
    if (int rc = check_tables("opt_adam_step", tensors, n_tensors, chunks, n_chunks)) return rc;
    Hyper h;
    if (int rc = make_hyper("opt_adam_step", hyper, &h)) return rc;
    SS_CHECK_ARG(tensor_scalars != nullptr, "opt_adam_step: null tensor_scalars");
    SS_CHECK_ARG(((uintptr_t)tensor_scalars & 3) == 0 && ((uintptr_t)grad_scale & 3) == 0,
                 "opt_adam_step: tensor_scalars and grad_scale must be 4-byte aligned");
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)std::min<int64_t>(n_chunks, kMaxWg)), dim3(kOT), 0, as_stream(stream), tensors, n_tensors,
                       chunks, (long long)n_chunks, h, tensor_scalars, grad_scale);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_grad_norm(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                         double* partials, int32_t* partial_flags, double max_norm, double* norm, float* coef, int32_t* flag,
                                         void* stream) {
    if (int rc = check_tables("opt_grad_norm", tensors, n_tensors, chunks, n_chunks)) return rc;
    SS_CHECK_ARG(partials && partial_flags && norm && coef && flag, "opt_grad_norm: null pointer");
    SS_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)norm & 7) == 0 && ((uintptr_t)partial_flags & 3) == 0 &&
                     ((uintptr_t)coef & 3) == 0 && ((uintptr_t)flag & 3) == 0,
                 "opt_grad_norm: partials and norm must be 8-byte aligned, partial_flags, coef and flag 4-byte aligned");
    SS_CHECK_ARG(max_norm == max_norm, "opt_grad_norm: max_norm is NaN (negative: no clip)");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3((unsigned)std::min<int64_t>(n_chunks, kMaxWg)), dim3(kOT), 0, s, tensors, n_tensors, chunks,
                       (long long)n_chunks, partials, partial_flags);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kOT), 0, s, partials, partial_flags, (long long)n_chunks, max_norm, norm, coef, flag);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_bucket_plan(const StemsegOptTensor* tensors_host, int32_t n_tensors, int64_t* offsets_host, int64_t* total) {
    SS_CHECK_ARG(tensors_host != nullptr && total != nullptr, "opt_bucket_plan: null pointer");
    SS_CHECK_ARG(n_tensors > 0, "opt_bucket_plan: n_tensors %d must be positive", n_tensors);
    int64_t at = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const int64_t n = tensors_host[t].n;
        SS_CHECK_ARG(n >= 0, "opt_bucket_plan: tensor %d has a negative element count %lld", t, (long long)n);
        SS_CHECK_ARG(n <= (1ll << 46) && at <= (1ll << 46), "opt_bucket_plan: more than 2^46 elements");
        if (offsets_host != nullptr) offsets_host[t] = at;
        at += round_up(n, 4);
    }
    *total = at;
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_pack_grads(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                          const int64_t* offsets, float* bucket, int64_t total, float scale, void* stream) {
    if (int rc = check_bucket("opt_pack_grads", tensors, n_tensors, chunks, n_chunks, offsets, bucket, total)) return rc;
    SS_CHECK_ARG(std::isfinite(scale), "opt_pack_grads: scale %g is not finite", (double)scale);
    const dim3 grid((unsigned)std::min<int64_t>(n_chunks, kMaxWg));
    const long long* off = reinterpret_cast<const long long*>(offsets);
    if (scale == 1.0f)
        hipLaunchKernelGGL(pack_grads_kernel<true>, grid, dim3(kOT), 0, as_stream(stream), tensors, n_tensors, chunks, (long long)n_chunks, off, bucket,
                           (long long)total, scale);
    else
        hipLaunchKernelGGL(pack_grads_kernel<false>, grid, dim3(kOT), 0, as_stream(stream), tensors, n_tensors, chunks, (long long)n_chunks, off, bucket,
                           (long long)total, scale);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_unpack_grads(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                            const int64_t* offsets, const float* bucket, int64_t total, void* stream) {
    if (int rc = check_bucket("opt_unpack_grads", tensors, n_tensors, chunks, n_chunks, offsets, bucket, total)) return rc;
    hipLaunchKernelGGL(unpack_grads_kernel, dim3((unsigned)std::min<int64_t>(n_chunks, kMaxWg)), dim3(kOT), 0, as_stream(stream), tensors, n_tensors,
                       chunks, (long long)n_chunks, reinterpret_cast<const long long*>(offsets), bucket, (long long)total);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_opt_reduce_ranks(const float* gathered, int32_t world, int64_t total, float* bucket, void* stream) {
    SS_CHECK_ARG(gathered != nullptr && bucket != nullptr, "opt_reduce_ranks: null pointer");
    SS_CHECK_ARG(world >= 1 && world <= STEMSEG_OPT_MAX_WORLD, "opt_reduce_ranks: world %d outside 1..%d", world, STEMSEG_OPT_MAX_WORLD);
    SS_CHECK_ARG(total > 0 && total <= (1ll << 46) / world, "opt_reduce_ranks: total %lld outside 1..2^46 / world", (long long)total);
    SS_CHECK_ARG((((uintptr_t)gathered | (uintptr_t)bucket) & 3) == 0, "opt_reduce_ranks: gathered and bucket must be 4-byte aligned");
    const uintptr_t lo = (uintptr_t)gathered, hi = lo + (uintptr_t)world * (uintptr_t)total * sizeof(float), b = (uintptr_t)bucket;
    SS_CHECK_ARG(b + (uintptr_t)total * sizeof(float) <= lo || b >= hi, "opt_reduce_ranks: the bucket lies inside the gathered buffer");
    const int64_t n_chunks = ceil_div(total, (int64_t)kChunk);
    const int vec = ((lo | b) & 15) == 0 && total % 4 == 0;
    hipLaunchKernelGGL(reduce_ranks_kernel, dim3((unsigned)std::min<int64_t>(n_chunks, kMaxWg)), dim3(kOT), 0, as_stream(stream), gathered, world,
                       (long long)total, bucket, (long long)n_chunks, vec);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
