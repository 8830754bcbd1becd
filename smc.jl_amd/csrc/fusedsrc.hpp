// fusedsrc.hpp - the text side of a FUSED run-time compiled likelihood (include/smcmi.h SMCMI_PROGRAM_FUSED): the user's function compiled
// into the generic mutation kernel, one launch per stage instead of three per MH step x block.  Pure host functions like progsrc.hpp - no
// HIP, no hiprtc - so that tests/fusedsrc_check.cpp can drive them on their own.
//
// The run-time compiler is handed one translation unit,
//     #line 1 "likelihood.hip"              the user's text: a message about its line k says likelihood.hip:k
//     #line 1 "smcmi_program_wrapper.hip"   the define that names the entry, #include "kernels.hpp", the wrapper kernel of the split path
//                                           (progsrc::wrapper_text, unchanged), the fused kernel smcmi_program_mutate, the ABI words
// and every header that unit can reach as a NAMED header: the project's own device headers, embedded at build time as string literals
// (embedded_headers.inc, written by the Makefile into the build directory: the text the compiler sees is the text the library itself was
// built from), and small stand-ins for the six system headers those include.  Nothing is read from the machine's include directories; a
// header the table lacks is an error.
#pragma once
#include <string>
#include <vector>

#include "progsrc.hpp"

namespace fusedsrc {

constexpr const char *MUTATE_NAME = "smcmi_program_mutate";
constexpr const char *ABI_NAME = "smcmi_program_abi";
constexpr const char *KERNELS_HEADER = "kernels.hpp";
constexpr int ABI_WORDS = 4;           // sizeof CloudPtrs, MutArgs, DevState, ModelDev as the run-time compiler laid them out

struct Header { const char *name, *text; };

// the project's device headers under the names their #include lines use
inline const std::vector<Header> &project_headers() {
    static const std::vector<Header> h = {
#include "embedded_headers.inc"
    };
    return h;
}

// What the project's headers include from the system, cut down to what they use of it.  The run-time compiler declares the HIP runtime, the
// device math functions and size_t by itself.
inline const std::vector<Header> &standin_headers() {
    static const std::vector<Header> h = {
        {"hip/hip_runtime.h", "// (the run-time compiler declares the HIP runtime by itself)\n"},
        {"stddef.h", "// (size_t: declared by the run-time compiler)\n"},
        {"stdint.h",
         "#pragma once\n"
         "typedef signed char int8_t;\ntypedef unsigned char uint8_t;\ntypedef short int16_t;\ntypedef unsigned short uint16_t;\n"
         "typedef int int32_t;\ntypedef unsigned int uint32_t;\ntypedef long long int64_t;\ntypedef unsigned long long uint64_t;\n"
         "typedef unsigned long uintptr_t;\ntypedef long intptr_t;\n"},
        {"math.h",
         "#pragma once\n"
         "#ifndef NAN\n#define NAN (__builtin_nanf(\"\"))\n#endif\n"
         "#ifndef INFINITY\n#define INFINITY (__builtin_inff())\n#endif\n"
         "#ifndef M_PI\n#define M_PI 3.14159265358979323846\n#endif\n"},
        {"type_traits",
         "#pragma once\n"
         "namespace std {\nusing __hip_internal::integral_constant;\nusing __hip_internal::is_same;\nusing __hip_internal::enable_if;\n}\n"},
        {"initializer_list",
         "#pragma once\n"
         "namespace std {\n"
         "template <class E> class initializer_list {\n"
         "    const E *b_;\n    size_t n_;\n"
         "    constexpr initializer_list(const E *b, size_t n) noexcept : b_(b), n_(n) {}\n"
         "public:\n"
         "    typedef E value_type;\n    typedef const E &reference;\n    typedef const E &const_reference;\n    typedef size_t size_type;\n"
         "    typedef const E *iterator;\n    typedef const E *const_iterator;\n"
         "    constexpr initializer_list() noexcept : b_(nullptr), n_(0) {}\n"
         "    constexpr size_t size() const noexcept { return n_; }\n"
         "    constexpr const E *begin() const noexcept { return b_; }\n"
         "    constexpr const E *end() const noexcept { return b_ + n_; }\n"
         "};\n"
         "template <class E> constexpr const E *begin(initializer_list<E> l) noexcept { return l.begin(); }\n"
         "template <class E> constexpr const E *end(initializer_list<E> l) noexcept { return l.end(); }\n"
         "}\n"},
    };
    return h;
}

// What a fused compile adds to progsrc::base_options(): the flag the library's own main translation unit is built with (Makefile MAINFLAGS).
// Hoisted address and constant computations otherwise stay in registers across the MH loop: the fused kernel for config 2's source has
// 164 VGPRs with machine LICM and 88 without (3 against 5 wavefronts per SIMD).  It moves instructions, never the value of one.
// -nostdinc -nostdinc++: without them the compiler searches the machine's include directories behind the named headers, and a source would
// compile or fail by what the host has installed; with them a header the table lacks ends in "file not found".
inline std::vector<std::string> extra_options() { return {"-nostdinc", "-nostdinc++", "-mllvm", "-disable-machine-licm"}; }

// In fused mode the caller's options reach the engine's mutation kernel, not the user's function alone.  Refused there (false, `why` says
// which): whatever adds an include path or a forced include (the header isolation), whatever touches floating-point contraction or fast
// math (the bits of the split path), and a define or undefine of one of the library's own names.
inline bool options_allowed(const std::vector<std::string> &opts, std::string *why) {
    for (const std::string &o : opts) {
        bool bad = false;
        for (const char *pre : {"-I", "-i", "--include", "--sysroot", "-stdlib", "-nostdinc", "-ffp-contract", "-ffast-math", "-funsafe-math", "-Ofast",
                                "-fno-fast-math", "-fassociative-math", "-freciprocal-math", "-fapprox-func", "-ffp-model", "-cl-", "-x", "-D__HIPCC_RTC__", "-U"})
            bad = bad || o.compare(0, std::char_traits<char>::length(pre), pre) == 0;
        bad = bad || o.find("SMCMI_") != std::string::npos;
        if (bad) {
            if (why) *why = "compiler option refused for a fused program (it would reach the engine's mutation kernel): " + o;
            return false;
        }
    }
    return true;
}

// every named header of a fused compile: the project's, then the stand-ins
inline std::vector<Header> header_table() {
    std::vector<Header> t = project_headers();
    t.insert(t.end(), standin_headers().begin(), standin_headers().end());
    return t;
}

// The fused kernel: k_mutate<0, 1>'s body (kernels.hpp mutate_kernel_body - the same text, with the user's function at the one place
// mutate_generic scores a proposal) and the wrapper kernel's evaluation count: one 64-bit atomic add per wavefront and launch.  The ABI words
// let the host refuse, at load, a code object whose structs are not the library's.
inline std::string mutate_text() {
    std::string w;
    w += "extern \"C\" __global__ void __launch_bounds__(256, 1) smcmi_program_mutate(\n";
    w += "        smcmi::CloudPtrs cl, const smcmi::DevState *st, const smcmi::ModelDev *md, smcmi::MutArgs ma, double *acc_partials, int standalone,\n";
    w += "        const double *data, long long rows, long long cols, const double *par, long long n_par, unsigned long long *evals) {\n";
    w += "    smcmi::ProgHook ph{data, rows, cols, par, n_par, 0ull};\n";
    w += "    smcmi::mutate_kernel_body<0, 1>(cl, st, md, ma, acc_partials, standalone, ph);\n";
    w += "    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);\n";
    w += "    if ((threadIdx.x & 63) == 0 && ph.scored != 0ull)\n";
    w += "        atomicAdd(evals + (wave % " + std::to_string(progsrc::EVAL_SLOTS) + "ull) * " + std::to_string(progsrc::EVAL_STRIDE) + "ull, ph.scored);\n";
    w += "}\n";
    w += "extern \"C\" __device__ __attribute__((used, visibility(\"default\"))) unsigned int smcmi_program_abi[4] = {\n";
    w += "    (unsigned int)sizeof(smcmi::CloudPtrs), (unsigned int)sizeof(smcmi::MutArgs), (unsigned int)sizeof(smcmi::DevState), (unsigned int)sizeof(smcmi::ModelDev)};\n";
    return w;
}

// `entry` has passed progsrc::valid_entry.  The Assembled fields mean what they mean in progsrc::assemble.
inline progsrc::Assembled assemble(const std::string &user, const std::string &entry) {
    progsrc::Assembled a;
    a.text = std::string("#line 1 \"") + progsrc::USER_FILE + "\"\n";
    a.user_first_line = 2;
    a.text += user;
    int lines = 0;
    for (char c : user) lines += c == '\n';
    if (!user.empty() && user.back() != '\n') { a.text += '\n'; ++lines; }
    a.user_lines = lines;
    a.wrapper_line_directive = a.user_first_line + lines;
    a.text += std::string("#line 1 \"") + progsrc::WRAPPER_FILE + "\"\n";
    // (::entry - inside namespace smcmi the library's own loglik would hide a user's function of that name; SMCMI_INST_UNIT - no host launchers)
    a.text += "#define SMCMI_PROGRAM_ENTRY ::" + entry + "\n";
    a.text += "#define SMCMI_INST_UNIT 1\n";
    a.text += std::string("#include \"") + KERNELS_HEADER + "\"\n";
    a.text += progsrc::wrapper_text(entry);
    a.text += mutate_text();
    return a;
}

}      // namespace fusedsrc
