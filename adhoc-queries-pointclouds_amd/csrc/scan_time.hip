// scan_time.hip — K3, the count-only fast path of the GPS time-range search.
//
// K3 time_count restates the predicate of _search_las_file_by_time_range_optimized (query/src/search/las.rs:335-338) over a
// packed column: the count of f64 GPS times with start <= t < end (Range<f64>::contains, IEEE: NaN is no match) in an 8-byte
// aligned block of N x f64 — a LAST time block, or one resident in HBM.  8 B/point, a pure streaming read, in K2's shape
// (scan_count.hip): one-wave workgroups, four per CU, persistent, software-pipelined by hand — 16-byte non-temporal loads of
// the next step (inline-asm global_load_dwordx4 nt + counted s_waitcnt) in flight while the current step is evaluated.  A
// load holds two times; each is compared per lane and counted per wave with a ballot and a popcount (a wave-uniform count),
// and every workgroup adds its count with one atomic.  A column that is not 8-byte aligned (or strided: LAS records) is
// counted by k_generic_count<PCQ_PRED_TIME> (scan_generic.hip).
#include "dev_common.h"
#include "scan_tiles.h"

using namespace pcqdev;

namespace {

constexpr int K3_LOADS = 4;         // 1 KiB loads per step: 512 times per wave and step
constexpr int K3_WAVES_PER_CU = 4;  // K2's measured shape (profiles/r01_k2_sweep.log)

__device__ __forceinline__ double f64_of(int lo, int hi) {
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
__device__ __forceinline__ bool in_range(double t, double t0, double t1) { return (t >= t0) & (t < t1); }
template <int LOADS>
__device__ __forceinline__ uint32_t time_eval(const VecRegs<LOADS> &R, double t0, double t1) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const double a = f64_of(R.r[k][0], R.r[k][1]), b = f64_of(R.r[k][2], R.r[k][3]);
        c += (uint32_t)__popcll(__ballot(in_range(a, t0, t1))) + (uint32_t)__popcll(__ballot(in_range(b, t0, t1)));
    }
    return c;
}

// `head` (0 or 1) times in front of the first 16-byte aligned one, nvec vectors of two times, at most one time behind them.
template <int LOADS>
__global__ __launch_bounds__(64) void k_time_count_pipe(const double *__restrict__ t, uint64_t n, double t0, double t1, uint64_t head,
                                                       uint64_t nvec, unsigned long long *__restrict__ d_count) {
    constexpr uint64_t STEP_VEC = 64 * LOADS;
    const int lane = threadIdx.x;
    const v4i *body = reinterpret_cast<const v4i *>(t + head);
    const uint64_t steps = nvec / STEP_VEC, stride = gridDim.x;
    uint32_t cnt = 0;  // (wave-uniform)
    if (blockIdx.x < steps) {
        VecRegs<LOADS> A, B;
        uint64_t u = blockIdx.x;
        vec_load(A, body + u * STEP_VEC, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            vec_load(B, body + (u1 < steps ? u1 : u) * STEP_VEC, lane);  // clamped at the tail: a re-read that hits L2
            pipe_wait<LOADS>(A);
            cnt += time_eval<LOADS>(A, t0, t1);
            if (u1 >= steps) break;
            const uint64_t u2 = u1 + stride;
            vec_load(A, body + (u2 < steps ? u2 : u1) * STEP_VEC, lane);
            pipe_wait<LOADS>(B);
            cnt += time_eval<LOADS>(B, t0, t1);
            if (u2 >= steps) break;
            u = u2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
    if (blockIdx.x == 0) {
        for (uint64_t v0 = steps * STEP_VEC; v0 < nvec; v0 += 64) {  // fewer than a step of leftover vectors
            const uint64_t v = v0 + lane;
            bool pa = false, pb = false;
            if (v < nvec) {
                const v4i q = body[v];
                pa = in_range(f64_of(q[0], q[1]), t0, t1);
                pb = in_range(f64_of(q[2], q[3]), t0, t1);
            }
            cnt += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
        }
        const uint64_t last = head + 2 * nvec;
        bool p = false;  // lane 0: the head time, lane 1: the tail time
        if (lane == 0 && head) p = in_range(t[0], t0, t1);
        if (lane == 1 && last < n) p = in_range(t[last], t0, t1);
        cnt += (uint32_t)__popcll(__ballot(p));
    }
    if (lane == 0 && cnt) atomicAdd(d_count, (unsigned long long)cnt);
}

}  // namespace

int pcq_launch_time_count_f64(pcq_ctx *ctx, const void *d_t, uint64_t n, const DevPred &pred, uint64_t *d_count, hipStream_t s) {
    if (n == 0) return PCQ_OK;
    if (((uintptr_t)d_t & 7) != 0) return pcq_fail(PCQ_ERR_ARG, "time_count_f64: time block must be 8-byte aligned");
    const uint64_t head = ((uintptr_t)d_t & 15) != 0 ? 1 : 0;
    const uint64_t nvec = (n - head) / 2;
    uint64_t g = (uint64_t)ctx->num_cus * K3_WAVES_PER_CU;
    const uint64_t steps = nvec / (64 * K3_LOADS) + 1;
    if (g > steps) g = steps;
    hipLaunchKernelGGL(k_time_count_pipe<K3_LOADS>, dim3((unsigned)g), dim3(64), 0, s, reinterpret_cast<const double *>(d_t), n, pred.wmin[0],
                       pred.wmax[0], head, nvec, reinterpret_cast<unsigned long long *>(d_count));
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}
