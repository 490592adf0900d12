// The device half of the KITTI-MOTS measures (stemseg_amd/evaluation/mots.py; the measure is DEFINED in include/stemseg_hip.h and
// restated by tests/mots_eval_oracle.py): label_pair_counts, the joint histogram of two uint16 label maps, frame by frame.
//   counts[t][i][j] = the number of pixels of frame t with a == i and b == j, 0 <= i <= Ka, 0 <= j <= Kb; a label above Ka (Kb) counts
//   as 0, so every frame's table sums to H * W, the areas are its marginals and an intersection is a cell.
// Two launches whatever the data:
//   fill  : every element of the tables = 0
//   count : a workgroup of 256 threads owns kPixelsPerBlock consecutive pixels of ONE frame and a (Ka + 1) x (Kb + 1) int32 table in LDS
//           (at most 64 x 64 = 16 KB).  Most pixels are the pair (0, 0) and a frame may be one pair throughout, so no wave sends 64 adds
//           to one LDS word: per step the wave takes the key of its first lane still waiting (a lane read of a wave-uniform lane index),
//           ballots the lanes that hold the same key, the leader adds their number with ONE LDS atomic, and the step repeats until no
//           lane waits -- one add per wave, step and distinct key.  The table then goes out with one global integer atomic per non-zero
//           cell.  Sums of ones: the tables are the same bits in every run.
// Every global read is at a pixel index below H * W of the block's own frame; every global add is at (t, i <= Ka, j <= Kb).
#include "common.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kPixelsPerBlock = 8192;          // 32 steps of the workgroup
constexpr int kMaxK = STEMSEG_LABEL_PAIR_MAX_LABELS;
constexpr int kMaxCells = (kMaxK + 1) * (kMaxK + 1);

__global__ void pair_fill_kernel(int* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 0;
}

__global__ __launch_bounds__(kThreads) void label_pair_counts_kernel(const unsigned short* __restrict__ a, const unsigned short* __restrict__ b,
                                                                     unsigned int HW, int blocks_per_frame, int Ka, int Kb,
                                                                     int* __restrict__ counts) {
    __shared__ int table[kMaxCells];
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = blockIdx.x / blocks_per_frame, chunk = blockIdx.x - t * blocks_per_frame;
    const int cols = Kb + 1, cells = (Ka + 1) * cols;
    for (int i = tid; i < cells; i += kThreads) table[i] = 0;
    __syncthreads();

    const unsigned short* fa = a + (long long)t * HW;
    const unsigned short* fb = b + (long long)t * HW;
    const unsigned int first = (unsigned int)chunk * kPixelsPerBlock;
    const unsigned int end = HW - first < (unsigned int)kPixelsPerBlock ? HW : first + kPixelsPerBlock;
    // every thread of the workgroup runs every step (the step count depends on the chunk alone), so the ballots see whole waves
    for (unsigned int base = first; base < end; base += kThreads) {
        const unsigned int i = base + tid;
        const bool live = i < end;
        int key = -1;
        if (live) {
            int la = fa[i], lb = fb[i];
            la = la > Ka ? 0 : la;
            lb = lb > Kb ? 0 : lb;
            key = la * cols + lb;
        }
        unsigned long long waiting = __ballot(live);
        while (waiting) {
            const int leader = __ffsll(waiting) - 1;                             // wave-uniform
            const int k = __builtin_amdgcn_readlane(key, leader);
            const unsigned long long same = __ballot(key == k);                  // (k >= 0: a lane that is not live holds -1)
            if (lane == leader) atomicAdd(&table[k], __popcll(same));
            waiting &= ~same;
        }
    }
    __syncthreads();
    int* out = counts + (long long)t * cells;
    for (int i = tid; i < cells; i += kThreads) {
        const int v = table[i];
        if (v) atomicAdd(&out[i], v);
    }
}

}  // namespace

extern "C" int64_t stemseg_hip_label_pair_counts_size(int32_t T, int32_t Ka, int32_t Kb) {
    if (T < 1 || Ka < 1 || Ka > kMaxK || Kb < 1 || Kb > kMaxK) return 0;
    return (int64_t)T * (Ka + 1) * (Kb + 1);
}

extern "C" int stemseg_hip_label_pair_counts(const uint16_t* a, const uint16_t* b, int32_t T, int32_t H, int32_t W, int32_t Ka, int32_t Kb,
                                             int32_t* counts, int64_t counts_size, void* stream) {
    SS_CHECK_ARG(a && b && counts, "label_pair_counts: null pointer");
    SS_CHECK_ARG(T >= 1 && H >= 1 && W >= 1, "label_pair_counts: bad dims T=%d H=%d W=%d", T, H, W);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "label_pair_counts: a frame of %d x %d exceeds 2^31 pixels", H, W);
    SS_CHECK_ARG(Ka >= 1 && Ka <= kMaxK, "label_pair_counts: Ka=%d labels, the limit is %d", Ka, kMaxK);
    SS_CHECK_ARG(Kb >= 1 && Kb <= kMaxK, "label_pair_counts: Kb=%d labels, the limit is %d", Kb, kMaxK);
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(a) % 2 == 0 && reinterpret_cast<uintptr_t>(b) % 2 == 0 && reinterpret_cast<uintptr_t>(counts) % 4 == 0,
                 "label_pair_counts: misaligned label maps (uint16) or tables (int32)");
    const int64_t need = stemseg_hip_label_pair_counts_size(T, Ka, Kb);
    SS_CHECK_ARG(counts_size >= need, "label_pair_counts: the tables hold %lld int32, %lld needed", (long long)counts_size, (long long)need);
    const long long HW = (long long)H * W, blocks_per_frame = ceil_div(HW, (long long)kPixelsPerBlock);
    SS_CHECK_ARG((long long)T * blocks_per_frame < (1ll << 31), "label_pair_counts: T=%d frames of %d x %d need more than 2^31 workgroups", T, H, W);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(pair_fill_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(need, (int64_t)kThreads), 1024))), dim3(kThreads),
                       0, s, counts, (long long)need);
    hipLaunchKernelGGL(label_pair_counts_kernel, dim3((unsigned)(T * blocks_per_frame)), dim3(kThreads), 0, s, a, b, (unsigned int)HW,
                       (int)blocks_per_frame, Ka, Kb, counts);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
