// prologue.hpp - a fresh run on one handle: ONE launch in front of its first stage, ONE host round trip behind its last (run2.hpp).
// Included by handle.hpp behind stage3.hpp; the instantiation units launch none of this.
#pragma once
#ifndef SMCMI_INST_UNIT
#include <cstddef>

namespace smcmi {

// The loop state a fresh run starts from is a handful of scalars in front of DevState::sol and zeros behind them: the scalars travel as a
// kernel argument, the zeros are written on the device.
constexpr size_t ST_HEAD_BYTES = offsetof(DevState, sol);
static_assert(ST_HEAD_BYTES % 8 == 0 && sizeof(DevState) % 8 == 0 && offsetof(DevState, cov) % 8 == 0, "DevState is copied as 8-byte words");
struct StateHead { unsigned long long w[ST_HEAD_BYTES / 8]; };
// What the end of a run hands the host in host-mapped memory: DevState as far as engines 2 / 3 write it - up to the n_para x n_para entries
// of cov, n_para <= 16 - then the stage counts of the run's segment launches.
constexpr int RES2_STATE_WORDS = (int)((offsetof(DevState, cov) + 16 * 16 * sizeof(double)) / 8);
constexpr int RES2_DONE_MAX = 64;               // (a run with more segment launches reads its counts with a copy)
constexpr int RES2_WORDS = RES2_STATE_WORDS + RES2_DONE_MAX / 2;
constexpr int res2_state_words(int d) { return (int)((offsetof(DevState, cov) + (size_t)d * d * sizeof(double)) / 8); }

// ---- the shift at the head of a chain (kernels.hpp center_scan / k_center_one) for the prologue launch: the same block rows of
// (-min, max) per column, the same rule - maxima do not depend on the order they are taken in - with the loads of CENTER_COLS columns in
// flight together and one barrier pair per CENTER_COLS columns - one round up to n_para 10 (center_scan: a memory round trip and two block
// reductions per column, 44 µs for 10 columns of 100 000 particles).
constexpr int CENTER_COLS = 10;
constexpr int PRO2_GROUPS = 16;                  // ticket groups of the prologue launch (k2_run_prologue): 1 + PRO2_GROUPS ticket words
constexpr int CENTER_LDS = 2 * MAXD > 2 * (TB / 64) * CENTER_COLS ? 2 * MAXD : 2 * (TB / 64) * CENTER_COLS;      // doubles
__device__ inline void center_scan_wide(const double *cloud, long long n, int d, int R, double *part, double *smem) {
    const double *w = cloud + (long long)(R - 1) * n;
    const double inf = __builtin_inf();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long beg, end;
    block_chunk(n, gridDim.x, blockIdx.x, beg, end);
    for (int a0 = 0; a0 < d; a0 += CENTER_COLS) {
        double nlo[CENTER_COLS], hi[CENTER_COLS];
#pragma unroll
        for (int q = 0; q < CENTER_COLS; ++q) nlo[q] = hi[q] = -inf;
        for (long long i = beg + threadIdx.x; i < end; i += TB) {
            const bool live = w[i] > 0.0;
            double v[CENTER_COLS];
#pragma unroll
            for (int q = 0; q < CENTER_COLS; ++q) v[q] = cloud[(long long)(a0 + q < d ? a0 + q : d - 1) * n + i];       // (unconditional: one round trip for all)
#pragma unroll
            for (int q = 0; q < CENTER_COLS; ++q)
                if (live && fabs(v[q]) < inf) { nlo[q] = fmax(nlo[q], -v[q]); hi[q] = fmax(hi[q], v[q]); }
        }
#pragma unroll
        for (int q = 0; q < CENTER_COLS; ++q)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { nlo[q] = fmax(nlo[q], __shfl_xor(nlo[q], off, 64)); hi[q] = fmax(hi[q], __shfl_xor(hi[q], off, 64)); }
        __syncthreads();                                   // (the round before has been read)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < CENTER_COLS; ++q) { smem[(wave * CENTER_COLS + q) * 2] = nlo[q]; smem[(wave * CENTER_COLS + q) * 2 + 1] = hi[q]; }
        }
        __syncthreads();
        if (threadIdx.x < 2 * CENTER_COLS && a0 + (int)(threadIdx.x >> 1) < d) {
            const int q = threadIdx.x >> 1, s = threadIdx.x & 1;
            double m = smem[q * 2 + s];
            for (int wv = 1; wv < TB / 64; ++wv) m = fmax(m, smem[(wv * CENTER_COLS + q) * 2 + s]);
            part[((long long)blockIdx.x * d + a0 + q) * 2 + s] = m;
        }
    }
}
// nb block rows (written by other blocks during this launch) -> shift[0 .. d); all TB threads of one block call.  A wavefront per (column, side):
// its lanes walk the rows, no barrier until every maximum stands in LDS.
// lds_shift: the first 16 of them again, for the import that follows (zero where no shift is taken).
__device__ inline void center_finish_wide(const double *part, int nb, int d, double *shift, double *smem, double *lds_shift) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    constexpr int NW = TB / 64, IT = 8;                   // (IT (column, side) pairs of a wavefront in flight together: n_para <= 16 in one round)
    for (int it0 = wave; it0 < 2 * d; it0 += NW * IT) {
        double m[IT];
#pragma unroll
        for (int j = 0; j < IT; ++j) m[j] = -__builtin_inf();
#pragma unroll 4
        for (int b = lane; b < nb; b += 64) {
            const double *row = part + (long long)b * 2 * d;
            double v[IT];
#pragma unroll
            for (int j = 0; j < IT; ++j) v[j] = __hip_atomic_load(row + (it0 + NW * j < 2 * d ? it0 + NW * j : it0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < IT; ++j) m[j] = fmax(m[j], v[j]);
        }
#pragma unroll
        for (int j = 0; j < IT; ++j) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m[j] = fmax(m[j], __shfl_xor(m[j], off, 64));
            if (lane == 0 && it0 + NW * j < 2 * d) smem[it0 + NW * j] = m[j];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < d) {
        const double s = center_rule(smem[2 * threadIdx.x], smem[2 * threadIdx.x + 1]);
        shift[threadIdx.x] = s;
        if (threadIdx.x < 16) lds_shift[threadIdx.x] = s;
    }
}

struct Pro2Args {
    DevState *st; Ctl2 *ctl; Records rec;
    StateHead head;                              // DevState in front of `sol` as start_state left it in the handle
    double ess0, c0, acc0;                       // the stage-1 records (runsetup.hpp first_records)
    int max_stages;                              // rec.resampled is cleared
    long long n;                                 // history kept: w[:,1] = 0, W[:,1] = the cloud's weights (W0); hist_w null: none kept
    double *hist_w, *hist_W; const double *W0;
    int *tick; int n_tick;                       // engine 2's ticket counters, cleared
    int *done3; int n_done3;                     // engine 3: the stage counts of the run's segment launches, cleared (null: no engine 3)
    unsigned long long *to3, to3_bound;          // ... its time-out words {0, bound} (null: none)
    Sel3Args *sel3_dst; Sel3Args sel3;           // ... what its selection needs (null: no selection inside the segments)
    double *sched; const double *sched_src; int n_phi;      // the proposed schedule, read from host-mapped memory
    const double *cloud; int d, R;               // the shift of the chain's first moments: block rows, ticket
    double *part; int *ticket; int center;       // center = 0 (development, SMCMI_CENTER=0): no shift is taken
};
// Everything a fresh run used to enqueue one by one in front of its first stage - the push of DevState, the schedule, the centre of the cloud,
// the first records and history columns, the import into Ctl2, cleared tickets and stage counts, engine 3's small inputs - in one launch and
// without a host copy.  All blocks clear and copy their share and scan their chunk of the cloud; the block that draws the last ticket sees
// all of it, derives the shift, writes the scalars and imports them (k2_state's to_ctl branch).  The 1 + PRO2_GROUPS ticket words are 0 before the
// launch and 0 again after it.
static __global__ void __launch_bounds__(TB) k2_run_prologue(Pro2Args a) {
    __shared__ double smem[CENTER_LDS];
    __shared__ unsigned long long s_head[ST_HEAD_BYTES / 8];       // (the import reads the scalars and the shift here: one thread's loads from
    __shared__ double s_shift[16];                                 // global memory, each behind its stores into Ctl2, were half of the launch)
    __shared__ int s_last;
    const long long tid = (long long)blockIdx.x * TB + threadIdx.x, nth = (long long)gridDim.x * TB;
    unsigned long long *stw = reinterpret_cast<unsigned long long *>(a.st);
    for (long long k = (long long)(ST_HEAD_BYTES / 8) + tid; k < (long long)(sizeof(DevState) / 8); k += nth) stw[k] = 0ull;
    for (long long k = tid; k < a.max_stages; k += nth) a.rec.resampled[k] = 0;
    for (long long k = tid; k < a.n_tick; k += nth) a.tick[k] = 0;
    if (a.done3) for (long long k = tid; k < a.n_done3; k += nth) a.done3[k] = 0;
    for (long long k = tid; k < a.n_phi; k += nth) a.sched[k] = a.sched_src[k];
    if (a.hist_w) for (long long k = tid; k < a.n; k += nth) { a.hist_w[k] = 0.0; a.hist_W[k] = a.W0[k]; }
    if (a.center) center_scan_wide(a.cloud, a.n, a.d, a.R, a.part, smem);
    __syncthreads();
    if (threadIdx.x == 0) {
        // tickets in two levels - a.ticket[1 + g] among the blocks b = g mod PRO2_GROUPS, a.ticket[0] among the groups' last blocks: the
        // atomics of hundreds of blocks on ONE word are served one after the other, a memory round trip each
        const int g = blockIdx.x % PRO2_GROUPS, gsize = ((int)gridDim.x - g + PRO2_GROUPS - 1) / PRO2_GROUPS;
        const int groups = (int)gridDim.x < PRO2_GROUPS ? (int)gridDim.x : PRO2_GROUPS;
        __threadfence();                                   // this block's stores before its ticket
        int last = 0;
        if (atomicAdd(a.ticket + 1 + g, 1) == gsize - 1) {
            a.ticket[1 + g] = 0;
            __threadfence();                               // (what the group's blocks wrote, seen through their tickets, before the group's)
            last = atomicAdd(a.ticket, 1) == groups - 1;
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // (constant indices: a kernel argument indexed by the thread number is first copied to scratch, by every thread of the launch)
#pragma unroll
    for (int k = 0; k < (int)(ST_HEAD_BYTES / 8); ++k)
        if ((int)threadIdx.x == k) { stw[k] = a.head.w[k]; s_head[k] = a.head.w[k]; }
    static_assert(ST_HEAD_BYTES / 8 <= TB, "one word of the head per thread");
    if (threadIdx.x < 16) s_shift[threadIdx.x] = 0.0;
    if (a.center) center_finish_wide(a.part, (int)gridDim.x, a.d, a.st->shift, smem, s_shift);
    if (threadIdx.x == 0) {
        if (a.to3) { a.to3[0] = 0ull; a.to3[1] = a.to3_bound; }
        if (a.sel3_dst) *a.sel3_dst = a.sel3;
        *a.ticket = 0;
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) k2_import_state(reinterpret_cast<const DevState *>(s_head), s_shift, a.ctl, a.rec, 1, a.ess0, a.c0, a.acc0);
}
// The end of a run: Ctl2 -> DevState (k2_state's export), then DevState as far as a run of engines 2 / 3 writes it and the stage counts of
// the segment launches into host-mapped memory: the host syncs once and reads them there - no copy of DevState, no copy of the counts.
static __global__ void __launch_bounds__(64) k2_run_result(DevState *st, const Ctl2 *ctl, unsigned long long *res, int st_words, const int *done3, int n_done) {
    if (threadIdx.x == 0) { k2_export_state(st, ctl); __threadfence(); }
    __syncthreads();
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(st);
    for (int k = threadIdx.x; k < st_words; k += 64) res[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int *dn = reinterpret_cast<int *>(res + RES2_STATE_WORDS);
    for (int k = threadIdx.x; k < n_done; k += 64) dn[k] = done3[k];
}

}      // namespace smcmi
#endif
