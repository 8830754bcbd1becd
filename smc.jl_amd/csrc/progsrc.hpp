// progsrc.hpp - the text side of a run-time compiled likelihood (include/smcmi.h smcmi_program_compile): what the compiler is handed and
// with which options.  Pure host functions - no HIP, no hiprtc - so that tests/progsrc_check.cpp can drive them on their own.
//
// The compiler sees   #line 1 "likelihood.hip" \n  <the user's text> \n  #line 1 "smcmi_program_wrapper.hip" \n  <the engine's kernel>:
// a message about the user's line k says likelihood.hip:k, whatever the wrapper's length and whether or not the text ends in a newline.
#pragma once
#include <string>
#include <vector>

namespace progsrc {

constexpr int ENTRY_MAX = 64;
constexpr const char *USER_FILE = "likelihood.hip";
constexpr const char *WRAPPER_FILE = "smcmi_program_wrapper.hip";
constexpr const char *KERNEL_NAME = "smcmi_program_kernel";
constexpr const char *DEFAULT_ENTRY = "loglik";
constexpr int BLOCK = 256;            // threads of a block of the wrapper kernel (the launch in program.hip uses the same number)
// the evaluation counter: EVAL_SLOTS 64-bit words EVAL_STRIDE words apart, wavefront w adds to word w % EVAL_SLOTS (program.hpp has the
// same two numbers for the host side; program.hip asserts that they agree)
constexpr int EVAL_SLOTS = 256, EVAL_STRIDE = 16;

// a C identifier of 1 .. ENTRY_MAX characters
inline bool valid_entry(const char *e) {
    if (!e || !*e) return false;
    int len = 0;
    for (const char *p = e; *p; ++p, ++len) {
        const char c = *p;
        const bool alpha = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_', digit = c >= '0' && c <= '9';
        if (!(alpha || (digit && p != e))) return false;
        if (len >= ENTRY_MAX) return false;
    }
    return true;
}

// The engine's kernel around the user's function ENTRY: one launch per score (csrc/devcallback.hpp eval_device_callback).  Rows whose gate is
// -Inf failed the bounds check and never reach the function (the reference never calls the likelihood after a ParamBoundsError,
// src/mutation.jl:93); NaN -> -Inf is the reference's try / catch.  Every lane of a wavefront takes the same number of turns of the row loop,
// so the ballot counts whole wavefronts; a wavefront adds up its turns and ends with ONE 64-bit atomic add, by lane 0 when the sum is not 0,
// to its word of the counter.  Plain C++ only.
inline std::string wrapper_text(const std::string &entry) {
    std::string w;
    w += "extern \"C\" __global__ void __launch_bounds__(256) smcmi_program_kernel(\n";
    w += "        const double *theta, const double *gate, long long n, long long ld, int d, const double *data, long long rows, long long cols,\n";
    w += "        const double *par, long long n_par, double *lik, unsigned long long *evals) {\n";
    w += "    const long long stride = (long long)gridDim.x * 256;\n";
    w += "    const double neg_inf = -__builtin_inf();\n";
    w += "    unsigned long long scored = 0ull;\n";
    w += "    for (long long base = (long long)blockIdx.x * 256; base < n; base += stride) {\n";
    w += "        const long long i = base + threadIdx.x;\n";
    w += "        bool called = false;\n";
    w += "        if (i < n) {\n";
    w += "            double v = neg_inf;\n";
    w += "            if (gate[i] != neg_inf) {\n";
    w += "                called = true;\n";
    w += "                v = " + entry + "(theta + i, ld, d, data, rows, cols, par, n_par);\n";
    w += "                if (v != v) v = neg_inf;\n";
    w += "            }\n";
    w += "            lik[i] = v;\n";
    w += "        }\n";
    w += "        scored += (unsigned long long)__popcll(__ballot(called));\n";
    w += "    }\n";
    w += "    const unsigned long long wave = (unsigned long long)blockIdx.x * 4ull + (threadIdx.x >> 6);\n";
    w += "    if ((threadIdx.x & 63) == 0 && scored != 0ull)\n";
    w += "        atomicAdd(evals + (wave % " + std::to_string(EVAL_SLOTS) + "ull) * " + std::to_string(EVAL_STRIDE) + "ull, scored);\n";
    w += "}\n";
    return w;
}

struct Assembled {
    std::string text;
    int user_first_line = 0;        // physical line (1-based) of the user's first line in `text`
    int user_lines = 0;             // lines the user's text occupies (an unterminated last line counts)
    int wrapper_line_directive = 0; // physical line of the wrapper's #line directive: user_first_line + user_lines
};
// `entry` has passed valid_entry
inline Assembled assemble(const std::string &user, const std::string &entry) {
    Assembled a;
    a.text = std::string("#line 1 \"") + USER_FILE + "\"\n";
    a.user_first_line = 2;
    a.text += user;
    int lines = 0;
    for (char c : user) lines += c == '\n';
    if (!user.empty() && user.back() != '\n') { a.text += '\n'; ++lines; }
    a.user_lines = lines;
    a.wrapper_line_directive = a.user_first_line + lines;
    a.text += std::string("#line 1 \"") + WRAPPER_FILE + "\"\n";
    a.text += wrapper_text(entry);
    return a;
}

// The library's own options, then the caller's, split at white space.  Refused (false, `why` says which): an option that names a target
// (offload-arch, mcpu, mxnack) or contains "xnack" - the library is gfx950-only and serves no XNACK-on code objects.
inline std::vector<std::string> base_options() { return {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"}; }
inline bool split_options(const char *options, std::vector<std::string> *out, std::string *why) {
    out->clear();
    if (!options) return true;
    std::string cur;
    auto flush = [&]() { if (!cur.empty()) { out->push_back(cur); cur.clear(); } };
    for (const char *p = options; *p; ++p) {
        const char c = *p;
        if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v') flush();
        else cur += c;
    }
    flush();
    for (const std::string &o : *out) {
        std::string low;
        for (char c : o) low += (c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : c;
        for (const char *bad : {"offload-arch", "mcpu", "mxnack", "xnack"})
            if (low.find(bad) != std::string::npos) {
                if (why) *why = "compiler option refused (the target is fixed: gfx950, no XNACK): " + o;
                out->clear();
                return false;
            }
    }
    return true;
}

}      // namespace progsrc
