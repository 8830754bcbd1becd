// enssrc.hpp - the text side of a run-time compiled likelihood FOR ENSEMBLES (include/smcmi.h smcmi_program_compile_ensemble): the user's
// function compiled into the ensemble kernel (ensbody.hpp), one launch and one workgroup per member for whole runs.  Pure host functions like
// progsrc.hpp and fusedsrc.hpp - no HIP, no hiprtc - so that tests/enssrc_check.cpp can drive them on their own.
//
// The run-time compiler is handed one translation unit,
//     #line 1 "likelihood.hip"              the user's text: a message about its line k says likelihood.hip:k
//     #line 1 "smcmi_program_wrapper.hip"   the defines that name the entry and ask for the ensemble body, #include "ensbody.hpp", the wrapper
//                                           kernel of the split path (progsrc::wrapper_text, unchanged), the kernel smcmi_program_ensemble =
//                                           kens_run<n_para>'s text with the user's function as the likelihood, the ABI words
// and the named headers of a fused compile (fusedsrc.hpp: the project's device headers as embedded at build time, stand-ins for the system
// headers) plus the two the ensemble kernel adds, ensbody.hpp and ensshape.hpp (embedded_ens_headers.inc, written by the Makefile).  Options,
// their refusals and the header isolation are fusedsrc's.
#pragma once
#include <string>
#include <vector>

#include "fusedsrc.hpp"

namespace enssrc {

constexpr const char *ENSEMBLE_NAME = "smcmi_program_ensemble";
constexpr const char *ABI_NAME = "smcmi_program_ens_abi";
constexpr const char *BODY_HEADER = "ensbody.hpp";
constexpr int ABI_WORDS = 4;           // sizeof EnsMember, EnsArgs, DevState, ModelDev as the run-time compiler laid them out
constexpr int PARA_MIN = 1, PARA_MAX = 10;      // the n_para the ensemble kernel exists for (ensshape.hpp ENS_MAX_D)

// the device headers the ensemble kernel adds to a fused compile's, under the names their #include lines use
inline const std::vector<fusedsrc::Header> &ensemble_headers() {
    static const std::vector<fusedsrc::Header> h = {
#include "embedded_ens_headers.inc"
    };
    return h;
}
// What an ensemble compile adds to progsrc::base_options(): the header isolation of a fused compile, and none of its code generation flags -
// the library builds its own ensemble kernels (ens.hip) with the plain flags too.
inline std::vector<std::string> extra_options() { return {"-nostdinc", "-nostdinc++", "-mllvm", "-disable-machine-licm"}; }

// every named header of an ensemble compile: the fused compile's, then the ensemble kernel's
inline std::vector<fusedsrc::Header> header_table() {
    std::vector<fusedsrc::Header> t = fusedsrc::header_table();
    t.insert(t.end(), ensemble_headers().begin(), ensemble_headers().end());
    return t;
}

// The ensemble kernel for n_para: ens_run_body<n_para> is kens_run<n_para>'s text (ensbody.hpp).  The ABI words let the host refuse, at load,
// a code object whose structs are not the library's.
inline std::string ensemble_text(int n_para) {
    std::string w;
    w += "extern \"C\" __global__ void __launch_bounds__(256) smcmi_program_ensemble(smcmi::EnsArgs a, const smcmi::EnsProg *progs) {\n";
    w += "    smcmi::ens_run_body<" + std::to_string(n_para) + ">(a, progs);\n";
    w += "}\n";
    w += "extern \"C\" __device__ __attribute__((used, visibility(\"default\"))) unsigned int smcmi_program_ens_abi[4] = {\n";
    w += "    (unsigned int)sizeof(smcmi::EnsMember), (unsigned int)sizeof(smcmi::EnsArgs), (unsigned int)sizeof(smcmi::DevState), (unsigned int)sizeof(smcmi::ModelDev)};\n";
    return w;
}

// `entry` has passed progsrc::valid_entry, n_para lies in PARA_MIN .. PARA_MAX.  The Assembled fields mean what they mean in progsrc::assemble.
inline progsrc::Assembled assemble(const std::string &user, const std::string &entry, int n_para) {
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
    a.text += "#define SMCMI_PROGRAM_ENS 1\n";
    a.text += "#define SMCMI_INST_UNIT 1\n";
    a.text += std::string("#include \"") + BODY_HEADER + "\"\n";
    a.text += progsrc::wrapper_text(entry);
    a.text += ensemble_text(n_para);
    return a;
}

}      // namespace enssrc
