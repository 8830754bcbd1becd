// enskernel.hpp - the host's launcher of the ensemble kernel (include/smcmi.h smcmi_run_ensemble): kens_run<n_para>, one workgroup per
// member.  The kernel itself - its structs, its reductions, its body - is ensbody.hpp, which depends on the device headers alone so that the
// run-time compiler can read it too (enssrc.hpp: a likelihood given as HIP source, compiled for ensembles).  Compiled per n_para in
// translation units of their own (ens.hip).
#pragma once
#include <cstddef>

#include "launch2.hpp"
#include "ensbody.hpp"

static_assert(smcmi::ENS_HEAD_BYTES == offsetof(smcmi::DevState, sol), "the member table carries what stands in front of DevState::sol");

// the launch of n_members workgroups; instantiated in ens.hip (one translation unit per n_para, built in parallel), extern everywhere else
template <int D>
int launch_kens(const smcmi::EnsArgs &a, int n_members, hipStream_t stream) {
    using namespace smcmi;
    const EnsShape sh = ens_shape(a.n, D);
    if (!sh.ok) return SMCMI_ERR_UNSUPPORTED;
    // (more than the default 64 KB of dynamic LDS per block beyond some 2 700 particles at n_para 10: opt in to what the largest cloud takes;
    // a function attribute belongs to the device's copy of the kernel, so it is set for the current device at every call)
    if (set_max_lds(kens_run<D>, (ens_shape(SMCMI_ENS_MAX_PARTS, D).lds_bytes + 1023) / 1024 * 1024)) return SMCMI_ERR_HIP;
    kens_run<D><<<(unsigned)n_members, (unsigned)sh.block, sh.lds_bytes, stream>>>(a);
    return hipGetLastError() == hipSuccess ? 0 : SMCMI_ERR_HIP;
}
#define SMCMI_LAUNCH_ENS_D(M, X) M(X, 1) M(X, 2) M(X, 3) M(X, 4) M(X, 5) M(X, 6) M(X, 7) M(X, 8) M(X, 9) M(X, 10)
#define SMCMI_LAUNCH_ENS_INSTANCE(X, D) X template int launch_kens<D>(const smcmi::EnsArgs &, int, hipStream_t);
#if defined(SMCMI_ENS_D)
SMCMI_LAUNCH_ENS_INSTANCE(, SMCMI_ENS_D)
#else
SMCMI_LAUNCH_ENS_D(SMCMI_LAUNCH_ENS_INSTANCE, extern)
#endif
