// summary.hpp - the kernels of the posterior summaries (csrc/summary.hip: weighted quantiles by selection, best particle).
// All of them are plain launches that read the cloud and write scratch memory of the call; none of them touches the handle's state.
//
// Geometry: blocks of TB threads, n_blocks(n) = clamp(ceil(n / (TB * ITEMS)), 1, MAX_BLOCKS) of them per column, each thread strides
// over the column by gridDim.x * TB.  Every floating-point sum follows one fixed tree - thread (ascending i), wavefront (shuffle-down
// 32, 16, .. 1), block (waves 0..3 in order), column (k_cand_final: 8 strided partial sums over the blocks, added 0..7) - which depends on n
// and this geometry only.  Minima, maxima and flags are integer operations (order-free), so they go through integer atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "quantsel.hpp"

namespace summary {

constexpr int TB = 256;
constexpr int ITEMS = 8;
constexpr int MAX_BLOCKS = 1024;
constexpr int SLOTS = quantsel::SLOTS;
constexpr int LEVELS = quantsel::MAX_LEVELS;
constexpr int FIN_SUB = TB / SLOTS;          // strided partial sums per slot in k_cand_final
typedef unsigned long long u64;

enum { FLAG_NAN_VALUE = 1, FLAG_BAD_WEIGHT = 2, FLAG_SOME_WEIGHT = 4 };

inline int n_blocks(long long n) {
    const long long b = (n + (long long)TB * ITEMS - 1) / ((long long)TB * ITEMS);
    return (int)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

__device__ inline u64 key_of(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__device__ inline u64 shfl_down_u64(u64 v, int off) {
    const int lo = __shfl_down((int)(unsigned)v, off, 64), hi = __shfl_down((int)(unsigned)(v >> 32), off, 64);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

// prepass: rec[4 k + 0] smallest key, [4 k + 1] largest key (particles with w ≠ 0), [4 k + 2] flags; the caller initialises {~0, 0, 0, 0}
__global__ __launch_bounds__(TB) void k_minmax(const double *__restrict__ cloud, long long n, int wcol, const int *__restrict__ cols,
                                               u64 *__restrict__ rec) {
    const int k = blockIdx.y;
    const double *x = cloud + (size_t)cols[k] * (size_t)n, *w = cloud + (size_t)wcol * (size_t)n;
    u64 kmin = ~0ull, kmax = 0ull, flags = 0ull;
    const long long stride = (long long)gridDim.x * TB;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
        const double xi = x[i], wi = w[i];
        if (xi != xi) flags |= FLAG_NAN_VALUE;
        if (!(wi >= 0.0) || wi == __builtin_inf()) flags |= FLAG_BAD_WEIGHT;
        else if (wi != 0.0) {
            const u64 key = key_of(xi);
            flags |= FLAG_SOME_WEIGHT;
            kmin = key < kmin ? key : kmin;
            kmax = key > kmax ? key : kmax;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const u64 a = shfl_down_u64(kmin, off), b = shfl_down_u64(kmax, off), c = shfl_down_u64(flags, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
        flags |= c;
    }
    if ((threadIdx.x & 63) == 0) {
        if (flags & FLAG_SOME_WEIGHT) {
            atomicMin(&rec[4 * k + 0], kmin);
            atomicMax(&rec[4 * k + 1], kmax);
        }
        if (flags) atomicOr(&rec[4 * k + 2], flags);
    }
}

// candidate pass: part[(k * gridDim.x + block) * SLOTS + j] = this block's share of S_j = Σ w·[key ≤ thr[k * SLOTS + j]].  One running sum
// per slot in registers: a 64-bit compare, a select and an FP64 add per (particle, slot); the thresholds are wave-uniform (scalar loads).
__global__ __launch_bounds__(TB) void k_cand(const double *__restrict__ cloud, long long n, int wcol, const int *__restrict__ cols,
                                             const u64 *__restrict__ thr, double *__restrict__ part) {
    __shared__ double sm[TB / 64][SLOTS];
    const int k = blockIdx.y;
    const double *x = cloud + (size_t)cols[k] * (size_t)n, *w = cloud + (size_t)wcol * (size_t)n;
    u64 t[SLOTS];
    double s[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) { t[j] = thr[(size_t)k * SLOTS + j]; s[j] = 0.0; }
    const long long stride = (long long)gridDim.x * TB;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
        const u64 key = key_of(x[i]);
        const double wi = w[i];
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) s[j] += key <= t[j] ? wi : 0.0;
    }
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        double v = s[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        s[j] = v;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) sm[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < SLOTS) {
        double v = sm[0][threadIdx.x];
        for (int q = 1; q < TB / 64; ++q) v += sm[q][threadIdx.x];
        part[((size_t)k * gridDim.x + blockIdx.x) * SLOTS + threadIdx.x] = v;
    }
}
// ... and the fixed-order sum over its nb blocks: S[k * SLOTS + j]
__global__ __launch_bounds__(TB) void k_cand_final(const double *__restrict__ part, int nb, double *__restrict__ S) {
    __shared__ double sm[FIN_SUB][SLOTS];
    const int k = blockIdx.x, j = threadIdx.x % SLOTS, sub = threadIdx.x / SLOTS;
    double v = 0.0;
    for (int b = sub; b < nb; b += FIN_SUB) v += part[((size_t)k * nb + b) * SLOTS + j];
    sm[sub][j] = v;
    __syncthreads();
    if (threadIdx.x < SLOTS) {
        double a = sm[0][j];
        for (int q = 1; q < FIN_SUB; ++q) a += sm[q][j];
        S[(size_t)k * SLOTS + j] = a;
    }
}

// finishing pass (and the prepass's w1): for LEVELS keys per column, among particles with w ≠ 0, wmin[k * LEVELS + l] = the bits of the smallest
// weight at keys[..] (weights are positive here, so their bit patterns order like their values) and prev1[..] = the largest key below it + 1.
// The caller initialises wmin to ~0 (none) and prev1 to 0 (none).
__global__ __launch_bounds__(TB) void k_atkey(const double *__restrict__ cloud, long long n, int wcol, const int *__restrict__ cols,
                                              const u64 *__restrict__ keys, u64 *__restrict__ wmin, u64 *__restrict__ prev1) {
    const int k = blockIdx.y;
    const double *x = cloud + (size_t)cols[k] * (size_t)n, *w = cloud + (size_t)wcol * (size_t)n;
    u64 K[LEVELS], wm[LEVELS], pv[LEVELS];
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) { K[l] = keys[(size_t)k * LEVELS + l]; wm[l] = ~0ull; pv[l] = 0ull; }
    const long long stride = (long long)gridDim.x * TB;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
        const double wi = w[i];
        if (wi != 0.0) {
            const u64 key = key_of(x[i]), wb = (u64)__double_as_longlong(wi);
#pragma unroll
            for (int l = 0; l < LEVELS; ++l) {
                if (key == K[l]) wm[l] = wb < wm[l] ? wb : wm[l];
                if (key < K[l]) pv[l] = key + 1 > pv[l] ? key + 1 : pv[l];
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) {
        u64 a = wm[l], b = pv[l];
        for (int off = 32; off > 0; off >>= 1) {
            const u64 a2 = shfl_down_u64(a, off), b2 = shfl_down_u64(b, off);
            a = a2 < a ? a2 : a;
            b = b2 > b ? b2 : b;
        }
        if ((threadIdx.x & 63) == 0) {
            if (a != ~0ull) atomicMin(&wmin[(size_t)k * LEVELS + l], a);
            if (b != 0ull) atomicMax(&prev1[(size_t)k * LEVELS + l], b);
        }
    }
}

// best particle: argmax of loglh (with_prior = 0) or loglh + logprior over (key of the criterion, index) pairs - a NaN ranks above everything,
// the lowest index wins among equal keys.  bkey / bidx: one pair per block.
__device__ inline void best_of(u64 &key, long long &idx, u64 key2, long long idx2) {
    if (key2 > key || (key2 == key && idx2 < idx)) { key = key2; idx = idx2; }
}
__device__ inline double criterion(const double *cloud, long long n, int d, int with_prior, long long i) {
    const double lh = cloud[(size_t)d * (size_t)n + (size_t)i];
    return with_prior ? lh + cloud[(size_t)(d + 1) * (size_t)n + (size_t)i] : lh;
}
__device__ inline void best_block(u64 &key, long long &idx, u64 (*smk)[1], long long (*smi)[1]) {
    for (int off = 32; off > 0; off >>= 1) {
        const u64 k2 = shfl_down_u64(key, off);
        const long long i2 = (long long)shfl_down_u64((u64)idx, off);
        best_of(key, idx, k2, i2);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smk[wave][0] = key; smi[wave][0] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < TB / 64; ++q) best_of(key, idx, smk[q][0], smi[q][0]);
}
__global__ __launch_bounds__(TB) void k_best(const double *__restrict__ cloud, long long n, int d, int with_prior, u64 *__restrict__ bkey,
                                             long long *__restrict__ bidx) {
    __shared__ u64 smk[TB / 64][1];
    __shared__ long long smi[TB / 64][1];
    u64 key = 0ull;
    long long idx = 0x7fffffffffffffffll;               // (no particle: loses against every real pair, also one whose key is 0)
    const long long stride = (long long)gridDim.x * TB;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
        const double c = criterion(cloud, n, d, with_prior, i);
        best_of(key, idx, c != c ? ~0ull : key_of(c), i);
    }
    best_block(key, idx, smk, smi);
    if (threadIdx.x == 0) { bkey[blockIdx.x] = key; bidx[blockIdx.x] = idx; }
}
// ... the winner over the nb blocks, its criterion and its d parameters: out[0] = index (as an integer's bits), out[1] = value, out[2 + j] = parameter j
__global__ __launch_bounds__(TB) void k_best_final(const double *__restrict__ cloud, long long n, int d, int with_prior, const u64 *__restrict__ bkey,
                                                   const long long *__restrict__ bidx, int nb, double *__restrict__ out) {
    __shared__ u64 smk[TB / 64][1];
    __shared__ long long smi[TB / 64][1];
    u64 key = 0ull;
    long long idx = 0x7fffffffffffffffll;
    for (int b = threadIdx.x; b < nb; b += TB) best_of(key, idx, bkey[b], bidx[b]);
    best_block(key, idx, smk, smi);
    if (threadIdx.x == 0) {
        out[0] = __longlong_as_double(idx);
        out[1] = criterion(cloud, n, d, with_prior, idx);
        for (int j = 0; j < d; ++j) out[2 + j] = cloud[(size_t)j * (size_t)n + (size_t)idx];
    }
}

}      // namespace summary
