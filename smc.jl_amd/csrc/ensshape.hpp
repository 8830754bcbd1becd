// ensshape.hpp - the launch shape of an ensemble member (enskernel.hpp kens_run: one workgroup = one whole SMC run), as a pure function
// of (n_parts, n_para): the block, how many particles a thread loops over, the dynamic LDS.  Plain C++17, no HIP: the driver
// (runens.hpp), the kernel and tests/ensemble_check.cpp read the same text.
#pragma once
#include "ldslayout.hpp"

namespace smcmi {

constexpr int ENS_T = 256;                   // threads of a member's workgroup (= TB: the block reductions of kernels.hpp are written for it)
constexpr int ENS_MAX_D = 10;                // the register mutation body (mh_draw / mh_step) exists for n_para <= 10
constexpr size_t ENS_STATIC_LDS = 1024;      // a bound on the kernel's static __shared__ words (the staged state head and a few scalars)

struct EnsShape {
    int ok;                                  // 0: refused (n_parts outside 1..SMCMI_ENS_MAX_PARTS, n_para outside 1..ENS_MAX_D, or no room in a CU's LDS)
    int block;                               // threads per workgroup
    int per_thread;                          // particles a thread loops over: ceil(n_parts / block)
    size_t lds_bytes;                        // dynamic LDS of the launch (lds::ens)
};
constexpr EnsShape ens_shape(long long n_parts, int n_para) {
    if (n_parts < 1 || n_parts > SMCMI_ENS_MAX_PARTS || n_para < 1 || n_para > ENS_MAX_D) return EnsShape{0, 0, 0, 0};
    const size_t bytes = lds::ens(n_para, n_parts).bytes;
    if (bytes + ENS_STATIC_LDS > CU_LDS_BYTES) return EnsShape{0, 0, 0, 0};
    return EnsShape{1, ENS_T, (int)((n_parts + ENS_T - 1) / ENS_T), bytes};
}
// The two ways a workgroup walks its particles.  Strided: trip q of thread t is particle q * block + t (the per-particle phases: loads
// and stores coalesce); -1 beyond the cloud.
constexpr long long ens_particle(const EnsShape &s, long long n_parts, int t, int q) {
    const long long p = (long long)q * s.block + t;
    return p < n_parts ? p : -1;
}
// Contiguous: thread t owns [beg, end) (the cumulative weights of a selection: a thread scans its own stretch serially)
constexpr void ens_chunk(const EnsShape &s, long long n_parts, int t, long long &beg, long long &end) {
    beg = (long long)t * s.per_thread;
    end = beg + s.per_thread;
    if (beg > n_parts) beg = n_parts;
    if (end > n_parts) end = n_parts;
}

}  // namespace smcmi
