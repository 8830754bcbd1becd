// program.hpp - likelihoods compiled at run time from HIP source (include/smcmi.h smcmi_program_*, csrc/program.hip): what the main
// translation unit needs of them.  No kernel lives here or in program.hip - the only device code is the text csrc/progsrc.hpp assembles.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// a compiled program: host memory only, tied to no handle and no device
struct smcmi_program {
    bool ok = false;                 // compiled: `code` holds a gfx950 code object with the wrapper kernel
    std::string entry;
    std::string log;                 // the compiler's log ("" when clean)
    std::vector<char> code;
};

namespace program {

// SMCMI_OK / _ERR_ARG / _ERR_UNSUPPORTED (no libhiprtc) / _ERR_COMPILE; *out is set for OK and ERR_COMPILE; `err` gets the message
int compile(const char *source, const char *entry, const char *options, smcmi_program **out, std::string *err);

// one program loaded on the current device: the handle's own module (hipModule_t / hipFunction_t behind void *)
struct Loaded {
    void *module = nullptr, *kernel = nullptr;
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

}      // namespace program
