// program.hpp - likelihoods compiled at run time from HIP source (include/smcmi.h smcmi_program_*, csrc/program.hip): what the main
// translation unit needs of them.  No kernel lives here or in program.hip - the only device code is the text csrc/progsrc.hpp assembles.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// a compiled program: host memory only, tied to no handle and no device
struct smcmi_program {
    bool ok = false;                 // compiled: `code` holds a gfx950 code object with the wrapper kernel
    bool fused = false;              // ... and the fused mutation kernel (SMCMI_PROGRAM_FUSED, csrc/fusedsrc.hpp)
    int32_t ens_para = 0;            // ... or, not 0, the ensemble kernel for this n_para (smcmi_program_compile_ensemble, csrc/enssrc.hpp)
    unsigned long long id = 0;       // a hash of the code object's bytes, taken at compile
    std::string entry;
    std::string log;                 // the compiler's log ("" when clean)
    std::vector<char> code;
};

namespace program {

// SMCMI_OK / _ERR_ARG / _ERR_UNSUPPORTED (no libhiprtc) / _ERR_COMPILE; *out is set for OK and ERR_COMPILE; `err` gets the message
// flags: 0 or SMCMI_PROGRAM_FUSED; any other bit is SMCMI_ERR_ARG
// ens_para != 0 (with flags = 0): an ensemble compile for that n_para; outside 1..10 it is SMCMI_ERR_ARG
int compile(const char *source, const char *entry, const char *options, int32_t flags, smcmi_program **out, std::string *err, int32_t ens_para = 0);

// one program loaded on the current device: the handle's own module (hipModule_t / hipFunction_t behind void *)
// (a fused program: also the fused mutation kernel, and the sizes its code object states for CloudPtrs, MutArgs, DevState and ModelDev -
// the main translation unit, which has those structs, compares them with its own before it keeps the module)
// (an ensemble program: the ensemble kernel, the n_para it was compiled for, the sizes its code object states for EnsMember, EnsArgs, DevState
// and ModelDev, compared the same way; id: the program's hash - members of one smcmi_run_ensemble call carry the same code object)
struct Loaded {
    void *module = nullptr, *kernel = nullptr, *mutate = nullptr, *ensemble = nullptr;
    unsigned abi[4] = {0, 0, 0, 0}, ens_abi[4] = {0, 0, 0, 0};
    int32_t ens_para = 0;
    unsigned long long id = 0;
};
int load(const smcmi_program *p, Loaded *out, std::string *err);       // SMCMI_OK / _ERR_HIP
void unload(Loaded *l);

// The evaluation counter of a handle is EVAL_SLOTS 64-bit words, EVAL_STRIDE words (128 bytes) apart: a wavefront adds its count to the
// word of its own number modulo EVAL_SLOTS, the host adds the words when it reads them (once per run).  One word for every wavefront
// of the chip cost 11 ns per atomic - at N = 10^6 more than the launches the fused kernel saves.
constexpr int EVAL_SLOTS = 256, EVAL_STRIDE = 16, EVAL_WORDS = EVAL_SLOTS * EVAL_STRIDE;

// blocks of one launch over n rows: grid-stride, at most ceil(n / 256) - what the device callback's count kernel launches - and at most 2048
unsigned grid_for(long long n);
struct Args {
    const double *theta, *gate;
    long long n, ld;
    int d;
    const double *data;
    long long rows, cols;
    const double *par;
    long long n_par;
    double *lik;
    unsigned long long *evals;
};
// enqueues the wrapper kernel on `stream` (a hipStream_t); returns the hipError_t as an int (0 = success)
int launch(const Loaded &l, const Args &a, void *stream);
// The fused mutation kernel on `stream`: grid x block threads, lds bytes of dynamic shared memory (the runtime does not gate a module's
// launch at 64 KiB); `args` are the kernel's twelve arguments in order (devcallback.hpp fused_mutation).  Returns the hipError_t as an int.
int launch_mutate(const Loaded &l, unsigned grid, unsigned block, size_t lds, void **args, void *stream);
// The ensemble kernel on `stream`, one block per member; `args` are its two arguments (runens.hpp).  Returns the hipError_t as an int.
int launch_ensemble(const Loaded &l, unsigned grid, unsigned block, size_t lds, void **args, void *stream);

}      // namespace program
