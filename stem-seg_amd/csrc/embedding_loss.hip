// Embedding loss (modeling/losses/embedding_loss.py:10-185 on the Lovasz hinge, _lovasz.py:51-63,130-147) and its gradient with respect
// to the head output, one sample per call, all instances of the sample batched as a grid dimension.
//
//   forward  (14 launches whatever I or P):
//     inst_partial / inst_final : per instance point count, sum of embeddings, of raw bandwidths and of exp(bw) * 10 (fp64 partial sums of
//                                 fp32 terms, fixed order); the background set and its seediness sum; the present list (nonzero().unique())
//     prob                      : p[n][v] of the n-th PRESENT instance's centre, the foreground seediness sum over that instance's points,
//                                 and the second pass of the smoothness term mean((mean_bw - bw)^2) of instance n itself
//     4 x (hist, scatter)       : stable LSD radix sort of ~bits(err) per instance, payload = voxel index: descending error, ties by
//                                 ascending voxel index.  err = 1 - (2p - 1) * sign >= 0, so its bit pattern is monotone.  Pass 0 computes
//                                 its keys from p and the mask.
//     lovasz_count / lovasz_apply: exact integer scan of the sorted labels (scan.h's block scan), jaccard in fp32 as the reference divides,
//                                 first differences, fp64 partial sums of relu(err) * grad, and the coefficient grad * [err > 0] scattered
//                                 back through the permutation for the backward pass
//     loss_final                : the sample's three terms (fp64) and its number of present instances
//   backward (3 launches): two per-instance reductions over all voxels (d/d centre, d/d mean activated bandwidth), their finalisation, and
//   one pass per voxel that sums every chain in a fixed order and writes each gradient element once.
// No floating-point atomics anywhere: two runs give identical bits.
#include "scan.h"

namespace stemseg {
namespace {

constexpr int kLT = 256;                 // threads per workgroup (= kScanThreads: block_exclusive_scan is shared)
constexpr int kRed = 64;                 // workgroups per instance in the grid-stride reductions
constexpr int kTile = 4096;              // items per workgroup in a radix pass and in the Lovasz scan (16 rounds of 256)
constexpr int kME = STEMSEG_MAX_EMB_DIMS;
static_assert(kLT == kScanThreads, "block_exclusive_scan is written for kScanThreads threads");

struct Dims {
    int E, B, I, F;                      // embedding dims, predicted bandwidth dims (E - free), instances, statistic fields 1 + E + 2B
    int nt;                              // tiles of kTile voxels
    long long P;
    float fb[kME];                       // bandwidth of embedding dim d >= B: fb[d - B]
};

struct InstRec {
    long long count;
    float mean_emb[kME], mean_bw[kME], mean_act[kME];
};
struct Head {
    int K;                               // present instances
    int n_kept;                          // n < K with masks[n] not empty
    long long bg_count;
    double bg_sum;
};

struct Ws {
    float *p, *coef;                     // [I][P]
    unsigned int *kA, *kB, *vA, *vB;     // [I][P]
    unsigned int *hist;                  // [I][nt][256]
    long long* tilecnt;                  // [I][nt]
    double *part;                        // [I + 1][kRed][F]
    double *tot;                         // [I + 1][F]
    double *seed_part, *smooth_part;     // [I][kRed]
    double *lov_part;                    // [I][nt]
    double *bpart;                       // [I][kRed][E + B]
    double *ar;                          // [I][E + B]
    InstRec* rec;                        // [I]
    int *pres, *kept;                    // [I]
    Head* head;
    size_t bytes;
};

Ws layout(const Dims& d, void* base) {
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n) { void* q = base ? (char*)base + off : nullptr; off += (size_t)round_up((int64_t)n, 256); return q; };
    const size_t IP = (size_t)d.I * (size_t)d.P;
    w.p = (float*)take(IP * 4);
    w.coef = (float*)take(IP * 4);
    w.kA = (unsigned int*)take(IP * 4);
    w.kB = (unsigned int*)take(IP * 4);
    w.vA = (unsigned int*)take(IP * 4);
    w.vB = (unsigned int*)take(IP * 4);
    w.hist = (unsigned int*)take((size_t)d.I * d.nt * 256 * 4);
    w.tilecnt = (long long*)take((size_t)d.I * d.nt * 8);
    w.part = (double*)take((size_t)(d.I + 1) * kRed * d.F * 8);
    w.tot = (double*)take((size_t)(d.I + 1) * d.F * 8);
    w.seed_part = (double*)take((size_t)d.I * kRed * 8);
    w.smooth_part = (double*)take((size_t)d.I * kRed * 8);
    w.lov_part = (double*)take((size_t)d.I * d.nt * 8);
    w.bpart = (double*)take((size_t)d.I * kRed * (d.E + d.B) * 8);
    w.ar = (double*)take((size_t)d.I * (d.E + d.B) * 8);
    w.rec = (InstRec*)take((size_t)d.I * sizeof(InstRec));
    w.pres = (int*)take((size_t)d.I * 4);
    w.kept = (int*)take((size_t)d.I * 4);
    w.head = (Head*)take(sizeof(Head));
    w.bytes = off;
    return w;
}

// sum over the workgroup in a fixed tree order; every thread gets the result
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int off = kLT / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ float err_of(float p, bool fg) {
    const float logit = p * 2.f - 1.f;
    return 1.f - logit * (fg ? 1.f : -1.f);
}

// ------------------------------------------------------------------------------------------------ instance statistics
__global__ __launch_bounds__(kLT) void inst_partial_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ masks,
                                                           const unsigned char* __restrict__ ignore, double* __restrict__ part) {
    __shared__ double sh[kLT];
    const int i = blockIdx.y;
    double acc[1 + 3 * kME];
#pragma unroll
    for (int f = 0; f < 1 + 3 * kME; ++f) acc[f] = 0.0;
    const long long P = d.P;
    if (i < d.I) {
        const unsigned char* m = masks + (long long)i * P;
        for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < P; v += (long long)kRed * kLT) {
            if (!m[v]) continue;
            acc[0] += 1.0;
#pragma unroll
            for (int e = 0; e < kME; ++e)
                if (e < d.E) acc[1 + e] += (double)x[(long long)e * P + v];
#pragma unroll
            for (int e = 0; e < kME; ++e)
                if (e < d.B) {
                    const float bw = x[(long long)(d.E + e) * P + v];
                    acc[1 + kME + e] += (double)bw;
                    acc[1 + 2 * kME + e] += (double)(expf(bw) * 10.f);
                }
        }
    } else {                             // the background set (masks == 0).all(0): ignored points are zeroed but still counted
        const float* seed = x + (long long)(d.E + d.B) * P;
        for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < P; v += (long long)kRed * kLT) {
            bool bg = true;
            for (int k = 0; k < d.I; ++k) bg = bg && !masks[(long long)k * P + v];
            if (!bg) continue;
            acc[0] += 1.0;
            if (!ignore[v]) {
                const float s = seed[v];
                acc[1] += (double)(s * s);
            }
        }
    }
    double* out = part + ((long long)i * kRed + blockIdx.x) * d.F;
    // field order of a row: count, E embedding sums, B raw bandwidth sums, B activated bandwidth sums
    for (int f = 0; f < d.F; ++f) {
        int src = f;
        if (f >= 1 + d.E + d.B) src = 1 + 2 * kME + (f - 1 - d.E - d.B);
        else if (f >= 1 + d.E) src = 1 + kME + (f - 1 - d.E);
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 1 + 3 * kME; ++q)
            if (q == src) v = acc[q];
        const double s = block_sum(v, sh);
        if (threadIdx.x == 0) out[f] = s;
    }
}

__global__ __launch_bounds__(kLT) void inst_final_kernel(Dims d, const double* __restrict__ part, double* __restrict__ tot, InstRec* __restrict__ rec,
                                                         int* __restrict__ pres, int* __restrict__ kept, Head* __restrict__ head) {
    const int n_items = (d.I + 1) * d.F;
    for (int it = threadIdx.x; it < n_items; it += kLT) {
        const int i = it / d.F, f = it % d.F;
        double s = 0.0;
        for (int b = 0; b < kRed; ++b) s += part[((long long)i * kRed + b) * d.F + f];
        tot[it] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int K = 0, nk = 0;
        for (int i = 0; i < d.I; ++i)
            if (tot[i * d.F] > 0.0) pres[K++] = i;
        for (int n = 0; n < d.I; ++n) {
            kept[n] = (n < K && tot[n * d.F] > 0.0) ? 1 : 0;
            nk += kept[n];
            if (n >= K) pres[n] = -1;
        }
        head->K = K;
        head->n_kept = nk;
        head->bg_count = (long long)tot[d.I * d.F];
        head->bg_sum = tot[d.I * d.F + 1];
    }
    for (int i = threadIdx.x; i < d.I; i += kLT) {
        const double* r = tot + i * d.F;
        InstRec o;
        o.count = (long long)r[0];
        const double inv = r[0] > 0.0 ? 1.0 / r[0] : 0.0;
        for (int e = 0; e < kME; ++e) {
            o.mean_emb[e] = e < d.E ? (float)(r[1 + e] * inv) : 0.f;
            o.mean_bw[e] = e < d.B ? (float)(r[1 + d.E + e] * inv) : 0.f;
            o.mean_act[e] = e < d.B ? (float)(r[1 + d.E + d.B + e] * inv) : 0.f;
        }
        rec[i] = o;
    }
}

// ------------------------------------------------------------------------------------------------ probabilities
__global__ __launch_bounds__(kLT) void prob_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ masks,
                                                   const InstRec* __restrict__ rec, const int* __restrict__ pres, const int* __restrict__ kept,
                                                   float* __restrict__ p_out, double* __restrict__ seed_part, double* __restrict__ smooth_part) {
    __shared__ double sh[kLT];
    const int n = blockIdx.y;
    const long long P = d.P;
    double seed_acc = 0.0, smooth_acc = 0.0;
    if (kept[n]) {                       // the n-th present instance's centre, paired with masks[n] later (the reference's index shift)
        const int j = pres[n];
        const InstRec r = rec[j];
        float c[kME], b[kME];
#pragma unroll
        for (int e = 0; e < kME; ++e) {
            c[e] = r.mean_emb[e];
            b[e] = e < d.B ? r.mean_act[e] : d.fb[e < d.B ? 0 : e - d.B];
        }
        const unsigned char* mj = masks + (long long)j * P;
        const float* seed = x + (long long)(d.E + d.B) * P;
        for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < P; v += (long long)kRed * kLT) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < kME; ++e)
                if (e < d.E) {
                    const float df = x[(long long)e * P + v] - c[e];
                    s += df * df * b[e];
                }
            const float p = expf(-0.5f * s);
            p_out[(long long)n * P + v] = p;
            if (mj[v]) {
                const float df = seed[v] - p;
                seed_acc += (double)(df * df);
            }
        }
    }
    const InstRec own = rec[n];
    if (own.count > 0) {                 // second pass of the smoothness term of instance n itself
        const unsigned char* m = masks + (long long)n * P;
        for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < P; v += (long long)kRed * kLT) {
            if (!m[v]) continue;
#pragma unroll
            for (int e = 0; e < kME; ++e)
                if (e < d.B) {
                    const float df = own.mean_bw[e] - x[(long long)(d.E + e) * P + v];
                    smooth_acc += (double)(df * df);
                }
        }
    }
    const double s1 = block_sum(seed_acc, sh);
    const double s2 = block_sum(smooth_acc, sh);
    if (threadIdx.x == 0) {
        seed_part[n * kRed + blockIdx.x] = s1;
        smooth_part[n * kRed + blockIdx.x] = s2;
    }
}

// ------------------------------------------------------------------------------------------------ segmented stable radix sort
template <bool FIRST>
__device__ __forceinline__ unsigned int load_key(const unsigned int* keys, const float* p, const unsigned char* m, long long i) {
    if (FIRST) return ~__float_as_uint(err_of(p[i], m[i] != 0));
    return keys[i];
}

template <bool FIRST>
__global__ __launch_bounds__(kLT) void sort_hist_kernel(long long P, int nt, const int* __restrict__ kept, const unsigned int* __restrict__ keys,
                                                        const float* __restrict__ p, const unsigned char* __restrict__ masks, int shift,
                                                        unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[256];
    const int n = blockIdx.y;
    if (!kept[n]) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long seg = (long long)n * P, base = (long long)blockIdx.x * kTile;
    for (int r = 0; r < kTile / kLT; ++r) {
        const long long i = base + r * kLT + threadIdx.x;
        if (i < P) atomicAdd(&h[(load_key<FIRST>(keys + seg, p + seg, masks + seg, i) >> shift) & 255], 1u);      // (integer, LDS)
    }
    __syncthreads();
    hist[((long long)n * nt + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

template <bool FIRST>
__global__ __launch_bounds__(kLT) void sort_scatter_kernel(long long P, int nt, const int* __restrict__ kept, const unsigned int* __restrict__ keys,
                                                           const unsigned int* __restrict__ vals, const float* __restrict__ p,
                                                           const unsigned char* __restrict__ masks, int shift, const unsigned int* __restrict__ hist,
                                                           unsigned int* __restrict__ keys_out, unsigned int* __restrict__ vals_out) {
    __shared__ long long sc[kLT];
    __shared__ unsigned int goff[256];
    __shared__ int running[256];
    __shared__ int wcnt[kLT / 64][256];
    const int n = blockIdx.y;
    if (!kept[n]) return;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    // where this tile's items of digit t start: all smaller digits of the segment, then digit t of the earlier tiles
    long long before = 0, total = 0;
    for (int b = 0; b < nt; ++b) {
        const unsigned int c = hist[((long long)n * nt + b) * 256 + t];
        if (b < (int)blockIdx.x) before += c;
        total += c;
    }
    long long all;
    const long long ex = block_exclusive_scan(total, sc, &all);
    goff[t] = (unsigned int)(ex + before);
    running[t] = 0;
    const long long seg = (long long)n * P, base = (long long)blockIdx.x * kTile;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int r = 0; r < kTile / kLT; ++r) {
        for (int w = 0; w < kLT / 64; ++w) wcnt[w][t] = 0;
        __syncthreads();
        const long long i = base + r * kLT + t;
        const bool valid = i < P;
        const unsigned int key = valid ? load_key<FIRST>(keys + seg, p + seg, masks + seg, i) : 0u;
        const int dg = (int)((key >> shift) & 255u);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1;
            const unsigned long long bb = __ballot(bit);
            same &= bit ? bb : ~bb;
        }
        if (valid && (same & lt) == 0) wcnt[wave][dg] = __popcll(same);      // the lowest lane of each digit group
        __syncthreads();
        if (valid) {
            int rank = running[dg] + __popcll(same & lt);
            for (int w = 0; w < wave; ++w) rank += wcnt[w][dg];
            const long long o = (long long)goff[dg] + rank;
            if (o < P) {
                keys_out[seg + o] = key;
                vals_out[seg + o] = FIRST ? (unsigned int)i : vals[seg + i];
            }
        }
        __syncthreads();
        int add = 0;
        for (int w = 0; w < kLT / 64; ++w) add += wcnt[w][t];
        running[t] += add;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ Lovasz gradient and dot
__global__ __launch_bounds__(kLT) void lovasz_count_kernel(long long P, int nt, const int* __restrict__ kept, const unsigned int* __restrict__ vals,
                                                           const unsigned char* __restrict__ masks, long long* __restrict__ tilecnt) {
    __shared__ long long sc[kLT];
    const int n = blockIdx.y;
    if (!kept[n]) return;
    const long long seg = (long long)n * P, base = (long long)blockIdx.x * kTile + (long long)threadIdx.x * (kTile / kLT);
    long long c = 0;
    for (int j = 0; j < kTile / kLT; ++j)
        if (base + j < P) c += masks[seg + vals[seg + base + j]] ? 1 : 0;
    long long total;
    block_exclusive_scan(c, sc, &total);
    if (threadIdx.x == 0) tilecnt[(long long)n * nt + blockIdx.x] = total;
}

__device__ __forceinline__ float jaccard_at(long long G, long long cum_gt, long long cum_not) {
    return 1.f - (float)(G - cum_gt) / (float)(G + cum_not);
}

__global__ __launch_bounds__(kLT) void lovasz_apply_kernel(long long P, int nt, const int* __restrict__ kept, const unsigned int* __restrict__ keys,
                                                           const unsigned int* __restrict__ vals, const unsigned char* __restrict__ masks,
                                                           const long long* __restrict__ tilecnt, float* __restrict__ coef, double* __restrict__ lov_part) {
    __shared__ long long sc[kLT];
    __shared__ double sh[kLT];
    const int n = blockIdx.y;
    if (!kept[n]) return;
    const int t = threadIdx.x;
    long long before = 0, all = 0;
    for (int b = t; b < nt; b += kLT) {
        const long long c = tilecnt[(long long)n * nt + b];
        if (b < (int)blockIdx.x) before += c;
        all += c;
    }
    long long G, tile_off;
    block_exclusive_scan(all, sc, &G);
    block_exclusive_scan(before, sc, &tile_off);
    const long long seg = (long long)n * P, base = (long long)blockIdx.x * kTile + (long long)t * (kTile / kLT);
    long long c = 0;
    for (int j = 0; j < kTile / kLT; ++j)
        if (base + j < P) c += masks[seg + vals[seg + base + j]] ? 1 : 0;
    long long tile_total;
    long long cum = tile_off + block_exclusive_scan(c, sc, &tile_total);      // labels set before position `base` of the sorted order
    double acc = 0.0;
    for (int j = 0; j < kTile / kLT; ++j) {
        const long long i = base + j;
        if (i >= P) break;
        const unsigned int v = vals[seg + i];
        const int gt = masks[seg + v] ? 1 : 0;
        const float prev = i > 0 ? jaccard_at(G, cum, i - cum) : 0.f;
        cum += gt;
        const float g = jaccard_at(G, cum, (i + 1) - cum) - prev;
        const float e = __uint_as_float(~keys[seg + i]);
        acc += (double)((e > 0.f ? e : 0.f) * g);
        if (v < P) coef[seg + v] = e > 0.f ? g : 0.f;
    }
    const double s = block_sum(acc, sh);
    if (t == 0) lov_part[(long long)n * nt + blockIdx.x] = s;
}

__global__ __launch_bounds__(kLT) void loss_final_kernel(Dims d, const InstRec* __restrict__ rec, const int* __restrict__ pres, const int* __restrict__ kept,
                                                         const Head* __restrict__ head, const double* __restrict__ lov_part,
                                                         const double* __restrict__ seed_part, const double* __restrict__ smooth_part,
                                                         double* __restrict__ out) {
    __shared__ double lov[kLT], sd[kLT], sm[kLT];
    double o_l = 0.0, o_s = 0.0, o_m = 0.0;
    for (int b0 = 0; b0 < d.I; b0 += kLT) {
        const int n = b0 + threadIdx.x;
        double l = 0.0, s = 0.0, m = 0.0;
        if (n < d.I) {
            if (kept[n]) {
                for (int b = 0; b < d.nt; ++b) l += lov_part[(long long)n * d.nt + b];
                for (int b = 0; b < kRed; ++b) s += seed_part[n * kRed + b];
                s /= (double)rec[pres[n]].count;
            }
            if (rec[n].count > 0) {
                for (int b = 0; b < kRed; ++b) m += smooth_part[n * kRed + b];
                m /= (double)rec[n].count * (double)d.B;
            }
        }
        lov[threadIdx.x] = l;
        sd[threadIdx.x] = s;
        sm[threadIdx.x] = m;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < kLT && b0 + k < d.I; ++k) {
                o_l += lov[k];
                o_s += sd[k];
                o_m += sm[k];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int K = head->K;
        if (K > 0) {
            out[0] = o_l;
            out[1] = o_m / (double)K;
            out[2] = o_s + head->bg_sum / (double)head->bg_count;
        } else {                         // no mask point: the reference skips the sample
            out[0] = out[1] = out[2] = 0.0;
        }
        out[3] = (double)K;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// per kept pair n: A[e] = sum_v w (x_e - c_e) beta_e  (d loss / d centre_e)   and   R[e] = sum_v w (-1/2) (x_e - c_e)^2  (d loss / d beta_e),
// w = coef * (-2 sign) * p  = d lovasz_n / d p * p, both before the upstream weight
__global__ __launch_bounds__(kLT) void bwd_partial_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ masks,
                                                          const InstRec* __restrict__ rec, const int* __restrict__ pres, const int* __restrict__ kept,
                                                          const float* __restrict__ p, const float* __restrict__ coef, double* __restrict__ bpart) {
    __shared__ double sh[kLT];
    const int n = blockIdx.y;
    if (!kept[n]) return;
    const long long P = d.P;
    const InstRec r = rec[pres[n]];
    double A[kME], R[kME];
#pragma unroll
    for (int e = 0; e < kME; ++e) A[e] = R[e] = 0.0;
    const unsigned char* m = masks + (long long)n * P;
    for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < P; v += (long long)kRed * kLT) {
        const float cf = coef[(long long)n * P + v];
        if (cf == 0.f) continue;
        const float w = cf * (m[v] ? -2.f : 2.f) * p[(long long)n * P + v];
#pragma unroll
        for (int e = 0; e < kME; ++e)
            if (e < d.E) {
                const float df = x[(long long)e * P + v] - r.mean_emb[e];
                const float be = e < d.B ? r.mean_act[e] : d.fb[e < d.B ? 0 : e - d.B];
                A[e] += (double)(w * df * be);
                if (e < d.B) R[e] += (double)(-0.5f * w * df * df);
            }
    }
    double* out = bpart + ((long long)n * kRed + blockIdx.x) * (d.E + d.B);
    for (int f = 0; f < d.E + d.B; ++f) {
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < kME; ++e) {
            if (e < d.E && f == e) v = A[e];
            if (e < d.B && f == d.E + e) v = R[e];
        }
        const double s = block_sum(v, sh);
        if (threadIdx.x == 0) out[f] = s;
    }
}

__global__ __launch_bounds__(kLT) void bwd_final_kernel(Dims d, const int* __restrict__ kept, const double* __restrict__ bpart, double* __restrict__ ar) {
    const int W = d.E + d.B;
    for (int it = threadIdx.x; it < d.I * W; it += kLT) {
        const int n = it / W, f = it % W;
        double s = 0.0;
        if (kept[n])
            for (int b = 0; b < kRed; ++b) s += bpart[((long long)n * kRed + b) * W + f];
        ar[it] = s;
    }
}

__global__ __launch_bounds__(kLT) void bwd_apply_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ masks,
                                                        const unsigned char* __restrict__ ignore, const InstRec* __restrict__ rec,
                                                        const int* __restrict__ pres, const int* __restrict__ kept, const Head* __restrict__ head,
                                                        const float* __restrict__ p, const float* __restrict__ coef, const double* __restrict__ ar,
                                                        const float* __restrict__ up, double total_instances, double batch, float* __restrict__ grad) {
    const long long P = d.P;
    const long long v = (long long)blockIdx.x * kLT + threadIdx.x;
    if (v >= P) return;
    const int K = head->K, C = d.E + d.B + 1, W = d.E + d.B;
    float gx[kME], gb[kME], gs = 0.f;
#pragma unroll
    for (int e = 0; e < kME; ++e) gx[e] = gb[e] = 0.f;
    if (K > 0) {
        const double g_l = (double)up[0] / total_instances;         // lovasz / total_instances (the per-instance factors: fp64, rounded once)
        const double g_m = (double)up[1] / batch / (double)K;       // smoothness: / present instances of the sample, / N
        const double g_s = (double)up[2] / (total_instances + 1.0); // seediness / (total_instances + 1)
        float xv[kME], bwv[kME];
#pragma unroll
        for (int e = 0; e < kME; ++e) {
            xv[e] = e < d.E ? x[(long long)e * P + v] : 0.f;
            bwv[e] = e < d.B ? x[(long long)(d.E + e) * P + v] : 0.f;
        }
        const float sv = x[(long long)W * P + v];
        bool bg = true;
        for (int n = 0; n < d.I; ++n) {
            const bool mn = masks[(long long)n * P + v] != 0;
            bg = bg && !mn;
            if (n < K && kept[n]) {
                const int j = pres[n];
                const InstRec& r = rec[j];
                const float pv = p[(long long)n * P + v];
                const float cf = coef[(long long)n * P + v];
                if (cf != 0.f) {                                   // through relu, err, logit and p to this voxel's embedding
                    const float w = (float)g_l * cf * (mn ? -2.f : 2.f) * pv;
#pragma unroll
                    for (int e = 0; e < kME; ++e)
                        if (e < d.E) {
                            const float be = e < d.B ? r.mean_act[e] : d.fb[e < d.B ? 0 : e - d.B];
                            gx[e] -= w * (xv[e] - r.mean_emb[e]) * be;
                        }
                }
                if (masks[(long long)j * P + v]) {                 // a point of the instance whose centre and mean bandwidth pair n uses
                    const double inv = g_l / (double)r.count;
#pragma unroll
                    for (int e = 0; e < kME; ++e) {
                        if (e < d.E) gx[e] += (float)(ar[n * W + e] * inv);
                        if (e < d.B) gb[e] += (float)(ar[n * W + d.E + e] * inv) * (expf(bwv[e]) * 10.f);
                    }
                    gs += (float)(2.0 * g_s / (double)r.count) * (sv - pv);      // the target p is detached
                }
            }
            if (mn) {                                              // smoothness of instance n itself (present, since this point is its)
                const InstRec& o = rec[n];
                const float sc = (float)(2.0 * g_m / ((double)o.count * (double)d.B));
#pragma unroll
                for (int e = 0; e < kME; ++e)
                    if (e < d.B) gb[e] += sc * (bwv[e] - o.mean_bw[e]);
            }
        }
        if (bg && !ignore[v]) gs += (float)(2.0 * g_s / (double)head->bg_count) * sv;
    }
    for (int e = 0; e < d.E; ++e) {
        float o = 0.f;
#pragma unroll
        for (int q = 0; q < kME; ++q)
            if (q == e) o = gx[q];
        grad[(long long)e * P + v] = o;
    }
    for (int e = 0; e < d.B; ++e) {
        float o = 0.f;
#pragma unroll
        for (int q = 0; q < kME; ++q)
            if (q == e) o = gb[q];
        grad[(long long)(d.E + e) * P + v] = o;
    }
    grad[(long long)(C - 1) * P + v] = gs;
}

int make_dims(const StemsegEmbeddingLossDesc* desc, Dims* d, const char* who) {
    SS_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
    SS_CHECK_ARG(desc->struct_bytes == (int32_t)sizeof(StemsegEmbeddingLossDesc), "%s: descriptor size mismatch (%d vs %d): ABI skew", who,
                 desc->struct_bytes, (int)sizeof(StemsegEmbeddingLossDesc));
    SS_CHECK_ARG(desc->embedding_size >= 1 && desc->embedding_size <= kME, "%s: embedding_size %d outside 1..%d", who, desc->embedding_size, kME);
    SS_CHECK_ARG(desc->n_free_dims >= 0 && desc->n_free_dims < desc->embedding_size, "%s: n_free_dims %d outside 0..embedding_size - 1", who,
                 desc->n_free_dims);
    SS_CHECK_ARG(desc->n_instances >= 1 && desc->n_instances <= 1024, "%s: n_instances %d outside 1..1024", who, desc->n_instances);
    SS_CHECK_ARG(desc->T >= 1 && desc->H >= 1 && desc->W >= 1, "%s: bad dims T %d H %d W %d", who, desc->T, desc->H, desc->W);
    const long long P = (long long)desc->T * desc->H * desc->W;
    SS_CHECK_ARG(P < (1ll << 24), "%s: T * H * W = %lld voxels, at most 2^24 - 1 (the label counts stay exact in fp32)", who, P);
    SS_CHECK_ARG(desc->reserved == 0, "%s: reserved must be 0", who);
    for (int k = 0; k < desc->n_free_dims; ++k)
        SS_CHECK_ARG(desc->free_dim_bandwidths[k] > 0.f, "%s: free_dim_bandwidths[%d] must be positive", who, k);
    d->E = desc->embedding_size;
    d->B = desc->embedding_size - desc->n_free_dims;
    d->I = desc->n_instances;
    d->F = 1 + d->E + 2 * d->B;
    d->P = P;
    d->nt = (int)ceil_div(P, kTile);
    for (int k = 0; k < kME; ++k) d->fb[k] = k < desc->n_free_dims ? desc->free_dim_bandwidths[k] : 0.f;
    return STEMSEG_OK;
}

}  // namespace
}  // namespace stemseg

using namespace stemseg;

extern "C" size_t stemseg_hip_embedding_loss_workspace_bytes(const StemsegEmbeddingLossDesc* desc) {
    Dims d;
    if (make_dims(desc, &d, "embedding_loss_workspace_bytes") != STEMSEG_OK) return 0;
    return layout(d, nullptr).bytes;
}

extern "C" int stemseg_hip_embedding_loss_forward(const StemsegEmbeddingLossDesc* desc, const float* embedding_map, const uint8_t* masks,
                                                  const uint8_t* ignore_masks, void* workspace, size_t ws_bytes, double* out,
                                                  int32_t* counts_host, void* stream) {
    Dims d;
    if (int rc = make_dims(desc, &d, "embedding_loss_forward")) return rc;
    SS_CHECK_ARG(embedding_map && masks && ignore_masks && workspace && out, "embedding_loss_forward: null pointer");
    SS_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "embedding_loss_forward: workspace must be 256-byte aligned");
    const Ws w = layout(d, workspace);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "embedding_loss_forward: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const dim3 blk(kLT), red(kRed, d.I), tiles(d.nt, d.I);
    hipLaunchKernelGGL(inst_partial_kernel, dim3(kRed, d.I + 1), blk, 0, s, d, embedding_map, masks, ignore_masks, w.part);
    hipLaunchKernelGGL(inst_final_kernel, dim3(1), blk, 0, s, d, w.part, w.tot, w.rec, w.pres, w.kept, w.head);
    hipLaunchKernelGGL(prob_kernel, red, blk, 0, s, d, embedding_map, masks, w.rec, w.pres, w.kept, w.p, w.seed_part, w.smooth_part);
    hipLaunchKernelGGL(sort_hist_kernel<true>, tiles, blk, 0, s, d.P, d.nt, w.kept, nullptr, w.p, masks, 0, w.hist);
    hipLaunchKernelGGL(sort_scatter_kernel<true>, tiles, blk, 0, s, d.P, d.nt, w.kept, nullptr, nullptr, w.p, masks, 0, w.hist, w.kA, w.vA);
    unsigned int *kin = w.kA, *vin = w.vA, *kout = w.kB, *vout = w.vB;
    for (int pass = 1; pass < 4; ++pass) {
        hipLaunchKernelGGL(sort_hist_kernel<false>, tiles, blk, 0, s, d.P, d.nt, w.kept, kin, nullptr, nullptr, 8 * pass, w.hist);
        hipLaunchKernelGGL(sort_scatter_kernel<false>, tiles, blk, 0, s, d.P, d.nt, w.kept, kin, vin, nullptr, nullptr, 8 * pass, w.hist, kout, vout);
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    // (three swaps: the sorted keys and voxel indices are in kB / vB, which `kin` / `vin` now name)
    hipLaunchKernelGGL(lovasz_count_kernel, tiles, blk, 0, s, d.P, d.nt, w.kept, vin, masks, w.tilecnt);
    hipLaunchKernelGGL(lovasz_apply_kernel, tiles, blk, 0, s, d.P, d.nt, w.kept, kin, vin, masks, w.tilecnt, w.coef, w.lov_part);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), blk, 0, s, d, w.rec, w.pres, w.kept, w.head, w.lov_part, w.seed_part, w.smooth_part, out);
    SS_LAUNCH_CHECK();
    if (counts_host) {                   // the one readback: the reference's skip rules and divisors depend on the counts
        Head h;
        SS_HIP(hipMemcpyAsync(&h, w.head, sizeof(Head), hipMemcpyDeviceToHost, s));
        SS_HIP(hipStreamSynchronize(s));
        counts_host[0] = h.K;
        counts_host[1] = h.n_kept;
    }
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_embedding_loss_backward(const StemsegEmbeddingLossDesc* desc, const float* embedding_map, const uint8_t* masks,
                                                   const uint8_t* ignore_masks, void* workspace, size_t ws_bytes, const float* upstream,
                                                   int32_t total_instances, int32_t batch_size, float* grad, void* stream) {
    Dims d;
    if (int rc = make_dims(desc, &d, "embedding_loss_backward")) return rc;
    SS_CHECK_ARG(embedding_map && masks && ignore_masks && workspace && upstream && grad, "embedding_loss_backward: null pointer");
    SS_CHECK_ARG(total_instances >= 1 && batch_size >= 1, "embedding_loss_backward: total_instances %d and batch_size %d must be positive",
                 total_instances, batch_size);
    SS_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "embedding_loss_backward: workspace must be 256-byte aligned");
    const Ws w = layout(d, workspace);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "embedding_loss_backward: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const dim3 blk(kLT);
    hipLaunchKernelGGL(bwd_partial_kernel, dim3(kRed, d.I), blk, 0, s, d, embedding_map, masks, w.rec, w.pres, w.kept, w.p, w.coef, w.bpart);
    hipLaunchKernelGGL(bwd_final_kernel, dim3(1), blk, 0, s, d, w.kept, w.bpart, w.ar);
    hipLaunchKernelGGL(bwd_apply_kernel, dim3((unsigned)ceil_div(d.P, kLT)), blk, 0, s, d, embedding_map, masks, ignore_masks, w.rec, w.pres, w.kept,
                       w.head, w.p, w.coef, w.ar, upstream, (double)total_instances, (double)batch_size, grad);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
