// The integer half of the DAVIS J and F measures (stemseg_amd/evaluation/davis.py; the arithmetic is DEFINED in include/stemseg_hip.h and
// restated by tests/davis_eval_oracle.py): for every frame t of a sequence, every proposal p (a label 1 .. Kp of the index map) and every
// ground-truth object g (a plane of `gt`), the counts from which the host divides J, precision and recall in fp64.
//
// One launch over (tiles in x, tiles in y, frames); a workgroup of 256 threads owns a TILE x TILE square of one frame and keeps in LDS
//   lab / gm : the label and the 32-bit membership word of the objects for the square grown by r (+ 1 to the south-east), coordinates
//              CLAMPED to the frame -- the clamped neighbours of the boundary rule are then plain neighbours in LDS;
//   bp / bg  : per position of the grown square the boundary words: bit p - 1 of the 64-bit word = a boundary pixel of proposal p, bit g
//              of the 32-bit word = of object g; zero outside the frame (there is nothing to dilate there).  From an index map a pixel
//              is on the boundary of at most the labels of its 2 x 2 neighbourhood: bits (l0) | (li) for every neighbour li != l0.
//   its own pixels then add the area / intersection / boundary counts into LDS tables and file the boundary pixels in a list; the
//   threads walk that list, OR the words over the disk dx^2 + dy^2 <= r^2 (the halo holds all of it) and add the matches; the tables go
//   out with one integer atomic per non-zero entry.
// Integers only: sums of ones do not depend on their order, so the tables are the same in every run.  A tile reads its own frame alone.
// Every global read is at clamped coordinates of that frame; every global add is at (t, p < Kp, g < Kg) of a table sized for them.
#include "common.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxKp = STEMSEG_DAVIS_EVAL_MAX_PROPOSALS, kMaxKg = STEMSEG_DAVIS_EVAL_MAX_OBJECTS, kMaxR = STEMSEG_DAVIS_EVAL_MAX_RADIUS;
constexpr int kMaxPairs = kMaxKp * kMaxKg;

struct Tables {          // the seven tables inside the caller's one buffer (stemseg_hip_davis_eval_counts_size)
    int *inter, *m_p, *m_g, *area_p, *n_p, *area_g, *n_g;
};

Tables carve(int* base, int T, int Kp, int Kg) {
    Tables t;
    const long long pairs = (long long)T * Kp * Kg, ps = (long long)T * Kp, gs = (long long)T * Kg;
    t.inter = base;
    t.m_p = t.inter + pairs;
    t.m_g = t.m_p + pairs;
    t.area_p = t.m_g + pairs;
    t.n_p = t.area_p + ps;
    t.area_g = t.n_p + ps;
    t.n_g = t.area_g + gs;
    return t;
}

__global__ void zero_tables_kernel(int* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 0;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// bit of proposal `l` (labels 1 .. Kp), nothing for the background (0 and everything above Kp)
__device__ __forceinline__ unsigned long long prop_bit(int l, int Kp) { return (l >= 1 && l <= Kp) ? 1ull << (l - 1) : 0ull; }

template <int TILE, int RMAX>
__global__ __launch_bounds__(kThreads) void davis_eval_kernel(const void* __restrict__ pred, int index_bytes, const unsigned char* __restrict__ gt,
                                                              int T, int H, int W, int Kp, int Kg, int r, Tables out) {
    constexpr int CAP = TILE + 2 * RMAX;          // side of the grown square at r = RMAX
    __shared__ unsigned long long bp[CAP * CAP];
    __shared__ unsigned int bg[CAP * CAP];
    __shared__ unsigned int gm[(CAP + 1) * (CAP + 1)];
    __shared__ unsigned short lab[(CAP + 1) * (CAP + 1)];
    __shared__ unsigned short list[TILE * TILE];
    __shared__ int s_inter[kMaxPairs], s_mp[kMaxPairs], s_mg[kMaxPairs];
    __shared__ int s_area_p[kMaxKp], s_np[kMaxKp], s_area_g[kMaxKg], s_ng[kMaxKg];
    __shared__ int half_width[2 * kMaxR + 1];
    __shared__ int n_list;

    const int tid = threadIdx.x, t = blockIdx.z;
    const int S = TILE + 2 * r, S1 = S + 1;          // r <= RMAX (the host picks the instance), so S <= CAP
    const int y0 = blockIdx.y * TILE - r, x0 = blockIdx.x * TILE - r;
    const int pairs = Kp * Kg;
    const long long HW = (long long)H * W;

    for (int i = tid; i < pairs; i += kThreads) s_inter[i] = s_mp[i] = s_mg[i] = 0;
    if (tid < kMaxKp) s_area_p[tid] = s_np[tid] = 0;
    if (tid < kMaxKg) s_area_g[tid] = s_ng[tid] = 0;
    if (tid <= 2 * r) {          // the disk's half width in row dy: the largest dx with dx^2 + dy^2 <= r^2
        const int dy = tid - r;
        int w = 0;
        while ((w + 1) * (w + 1) + dy * dy <= r * r) ++w;
        half_width[tid] = w;
    }
    if (tid == 0) n_list = 0;

    // labels and membership words at clamped coordinates
    for (int i = tid; i < S1 * S1; i += kThreads) {
        const int ay = i / S1, ax = i - ay * S1;
        const long long pix = (long long)clampi(y0 + ay, H - 1) * W + clampi(x0 + ax, W - 1);
        const long long at = (long long)t * HW + pix;
        lab[i] = index_bytes == 1 ? (unsigned short)static_cast<const unsigned char*>(pred)[at] : static_cast<const unsigned short*>(pred)[at];
        unsigned int m = 0;
        for (int g = 0; g < Kg; ++g) m |= (gt[((long long)g * T + t) * HW + pix] ? 1u : 0u) << g;
        gm[i] = m;
    }
    __syncthreads();

    // boundary words of the grown square; the counts of the tile's own pixels
    for (int i = tid; i < S * S; i += kThreads) {
        const int sy = i / S, sx = i - sy * S;
        const int y = y0 + sy, x = x0 + sx;
        unsigned long long wp = 0;
        unsigned int wg = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int a = sy * S1 + sx;
            const int l0 = lab[a], l1 = lab[a + 1], l2 = lab[a + S1], l3 = lab[a + S1 + 1];
            const unsigned long long b0 = prop_bit(l0, Kp);
            if (l1 != l0) wp |= b0 | prop_bit(l1, Kp);
            if (l2 != l0) wp |= b0 | prop_bit(l2, Kp);
            if (l3 != l0) wp |= b0 | prop_bit(l3, Kp);
            const unsigned int g0 = gm[a];
            wg = (g0 ^ gm[a + 1]) | (g0 ^ gm[a + S1]) | (g0 ^ gm[a + S1 + 1]);
            if (sy >= r && sy < r + TILE && sx >= r && sx < r + TILE) {          // one of the tile's own pixels
                const int p0 = (l0 >= 1 && l0 <= Kp) ? l0 - 1 : -1;
                if (p0 >= 0) atomicAdd(&s_area_p[p0], 1);
                for (unsigned int m = g0; m; m &= m - 1) {
                    const int g = __ffs(m) - 1;
                    atomicAdd(&s_area_g[g], 1);
                    if (p0 >= 0) atomicAdd(&s_inter[p0 * Kg + g], 1);
                }
                for (unsigned long long m = wp; m; m &= m - 1) atomicAdd(&s_np[__ffsll(m) - 1], 1);
                for (unsigned int m = wg; m; m &= m - 1) atomicAdd(&s_ng[__ffs(m) - 1], 1);
                if (wp | wg) list[atomicAdd(&n_list, 1)] = (unsigned short)i;
            }
        }
        bp[i] = wp;
        bg[i] = wg;
    }
    __syncthreads();

    // a boundary pixel of p counts for (p, g) when a boundary pixel of g lies within the disk around it, and the other way round
    const int n = n_list;
    for (int k = tid; k < n; k += kThreads) {
        const int i = list[k];
        const unsigned long long wp = bp[i];
        const unsigned int wg = bg[i];
        unsigned long long near_p = 0;
        unsigned int near_g = 0;
        for (int dy = -r; dy <= r; ++dy) {          // the pixel is the tile's own: every (dy, dx) of the disk stays inside the grown square
            const int w = half_width[dy + r], row = i + dy * S;
            for (int dx = -w; dx <= w; ++dx) {
                if (wg) near_p |= bp[row + dx];
                if (wp) near_g |= bg[row + dx];
            }
        }
        for (unsigned long long mp = wp; mp; mp &= mp - 1) {
            const int p = __ffsll(mp) - 1;
            for (unsigned int mg = near_g; mg; mg &= mg - 1) atomicAdd(&s_mp[p * Kg + __ffs(mg) - 1], 1);
        }
        for (unsigned int mg = wg; mg; mg &= mg - 1) {
            const int g = __ffs(mg) - 1;
            for (unsigned long long mp = near_p; mp; mp &= mp - 1) atomicAdd(&s_mg[(__ffsll(mp) - 1) * Kg + g], 1);
        }
    }
    __syncthreads();

    for (int i = tid; i < pairs; i += kThreads) {
        const long long at = (long long)t * pairs + i;
        if (s_inter[i]) atomicAdd(&out.inter[at], s_inter[i]);
        if (s_mp[i]) atomicAdd(&out.m_p[at], s_mp[i]);
        if (s_mg[i]) atomicAdd(&out.m_g[at], s_mg[i]);
    }
    if (tid < Kp) {
        if (s_area_p[tid]) atomicAdd(&out.area_p[(long long)t * Kp + tid], s_area_p[tid]);
        if (s_np[tid]) atomicAdd(&out.n_p[(long long)t * Kp + tid], s_np[tid]);
    }
    if (tid < Kg) {
        if (s_area_g[tid]) atomicAdd(&out.area_g[(long long)t * Kg + tid], s_area_g[tid]);
        if (s_ng[tid]) atomicAdd(&out.n_g[(long long)t * Kg + tid], s_ng[tid]);
    }
}

template <int TILE, int RMAX>
void launch(const void* pred, int index_bytes, const uint8_t* gt, int T, int H, int W, int Kp, int Kg, int r, const Tables& out, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(W, TILE), (unsigned)ceil_div(H, TILE), (unsigned)T);
    hipLaunchKernelGGL((davis_eval_kernel<TILE, RMAX>), grid, dim3(kThreads), 0, s, pred, index_bytes, gt, T, H, W, Kp, Kg, r, out);
}

}  // namespace

extern "C" int64_t stemseg_hip_davis_eval_counts_size(int32_t T, int32_t Kp, int32_t Kg) {
    if (T < 1 || T > STEMSEG_DAVIS_EVAL_MAX_FRAMES || Kp < 1 || Kp > kMaxKp || Kg < 1 || Kg > kMaxKg) return 0;
    return (int64_t)T * (3 * (int64_t)Kp * Kg + 2 * (int64_t)Kp + 2 * (int64_t)Kg);
}

extern "C" int stemseg_hip_davis_eval_counts(const void* pred, int32_t index_bytes, const uint8_t* gt, int32_t T, int32_t H, int32_t W, int32_t Kp,
                                             int32_t Kg, int32_t r, int32_t* counts, int64_t counts_size, void* stream) {
    SS_CHECK_ARG(pred && gt && counts, "davis_eval_counts: null pointer");
    SS_CHECK_ARG(index_bytes == 1 || index_bytes == 2, "davis_eval_counts: index_bytes=%d, the index map is uint8 (1) or uint16 (2)", index_bytes);
    SS_CHECK_ARG(T >= 1 && T <= STEMSEG_DAVIS_EVAL_MAX_FRAMES && H >= 1 && W >= 1, "davis_eval_counts: bad dims T=%d (at most %d) H=%d W=%d", T,
                 STEMSEG_DAVIS_EVAL_MAX_FRAMES, H, W);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "davis_eval_counts: a frame of %d x %d exceeds 2^31 pixels", H, W);
    SS_CHECK_ARG(H <= 16 * 65535, "davis_eval_counts: H=%d, at most %d rows", H, 16 * 65535);          // (tiles in y are a grid dimension)
    SS_CHECK_ARG(Kp >= 1 && Kp <= kMaxKp, "davis_eval_counts: Kp=%d proposals, the limit is %d", Kp, kMaxKp);
    SS_CHECK_ARG(Kg >= 1 && Kg <= kMaxKg, "davis_eval_counts: Kg=%d ground-truth objects, the limit is %d", Kg, kMaxKg);
    SS_CHECK_ARG(r >= 1 && r <= kMaxR, "davis_eval_counts: radius r=%d, the limits are 1 and %d", r, kMaxR);
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(pred) % index_bytes == 0 && reinterpret_cast<uintptr_t>(counts) % 4 == 0,
                 "davis_eval_counts: misaligned index map or tables");
    const int64_t need = stemseg_hip_davis_eval_counts_size(T, Kp, Kg);
    SS_CHECK_ARG(counts_size >= need, "davis_eval_counts: the tables hold %lld int32, %lld needed", (long long)counts_size, (long long)need);
    hipStream_t s = as_stream(stream);
    const Tables out = carve(counts, T, Kp, Kg);
    hipLaunchKernelGGL(zero_tables_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(need, kThreads), 1024))), dim3(kThreads), 0, s,
                       counts, (long long)need);
    // the tile shrinks as the halo grows, so that the grown square of boundary words stays in LDS
    if (r <= 8) launch<32, 8>(pred, index_bytes, gt, T, H, W, Kp, Kg, r, out, s);
    else if (r <= 16) launch<32, 16>(pred, index_bytes, gt, T, H, W, Kp, Kg, r, out, s);
    else launch<16, kMaxR>(pred, index_bytes, gt, T, H, W, Kp, Kg, r, out, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
