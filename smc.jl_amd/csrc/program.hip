// program.hip - likelihoods given as HIP source (include/smcmi.h smcmi_program_*): compile at run time, load on a handle's device, launch.
// A translation unit of its own, like summary.hip: nothing the engines' units compile depends on it, and it holds no kernel - the device
// code is the text of csrc/progsrc.hpp, compiled together with the user's function by the run-time compiler.
// libhiprtc is dlopen'ed the way sharded.hpp opens RCCL (hand-declared prototypes): libsmcmi.so has no link-time dependency on it, and a
// machine without it gets SMCMI_ERR_UNSUPPORTED from smcmi_program_compile and loses nothing else.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <mutex>

#include "../../include/smcmi.h"
#include "program.hpp"
#include "progsrc.hpp"
#include "fusedsrc.hpp"
#include "enssrc.hpp"

static_assert(program::EVAL_SLOTS == progsrc::EVAL_SLOTS && program::EVAL_STRIDE == progsrc::EVAL_STRIDE, "the wrapper text and the host disagree about the counter");

namespace {

// the eight entry points of the run-time compiler this unit uses (hiprtc.h: hiprtcResult is an enum, 0 = success; hiprtcProgram a pointer)
typedef void *rtc_prog;
struct Rtc {
    void *lib = nullptr;
    bool tried = false;
    std::string why;
    int (*CreateProgram)(rtc_prog *, const char *src, const char *name, int n_headers, const char **headers, const char **include_names) = nullptr;
    int (*CompileProgram)(rtc_prog, int n_options, const char **options) = nullptr;
    int (*GetProgramLogSize)(rtc_prog, size_t *) = nullptr;
    int (*GetProgramLog)(rtc_prog, char *) = nullptr;
    int (*GetCodeSize)(rtc_prog, size_t *) = nullptr;
    int (*GetCode)(rtc_prog, char *) = nullptr;
    int (*DestroyProgram)(rtc_prog *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
Rtc g_rtc;
std::mutex g_rtc_mutex;

bool rtc_open(std::string *err) {
    std::lock_guard<std::mutex> lock(g_rtc_mutex);
    if (!g_rtc.tried) {
        g_rtc.tried = true;
        for (const char *c : {"libhiprtc.so", "libhiprtc.so.7"}) {
            g_rtc.lib = dlopen(c, RTLD_NOW | RTLD_LOCAL);
            if (g_rtc.lib) break;
        }
        if (!g_rtc.lib) {
            const char *e = dlerror();
            g_rtc.why = std::string("cannot load the run-time compiler (libhiprtc): ") + (e ? e : "not found");
        } else {
#define SMCMI_RTC_SYM(field) *(void **)(&g_rtc.field) = dlsym(g_rtc.lib, "hiprtc" #field)
            SMCMI_RTC_SYM(CreateProgram); SMCMI_RTC_SYM(CompileProgram); SMCMI_RTC_SYM(GetProgramLogSize); SMCMI_RTC_SYM(GetProgramLog);
            SMCMI_RTC_SYM(GetCodeSize); SMCMI_RTC_SYM(GetCode); SMCMI_RTC_SYM(DestroyProgram); SMCMI_RTC_SYM(GetErrorString);
#undef SMCMI_RTC_SYM
            if (!g_rtc.CreateProgram || !g_rtc.CompileProgram || !g_rtc.GetProgramLogSize || !g_rtc.GetProgramLog || !g_rtc.GetCodeSize ||
                !g_rtc.GetCode || !g_rtc.DestroyProgram) {
                g_rtc.why = "libhiprtc lacks an entry point of the run-time compiler";
                dlclose(g_rtc.lib);
                g_rtc.lib = nullptr;
            }
        }
    }
    if (!g_rtc.lib && err) *err = g_rtc.why;
    return g_rtc.lib != nullptr;
}
std::string rtc_text(int code) {
    const char *s = g_rtc.GetErrorString ? g_rtc.GetErrorString(code) : nullptr;
    return s ? std::string(s) : "hiprtc error " + std::to_string(code);
}

}      // namespace

namespace program {

int compile(const char *source, const char *entry, const char *options, int32_t flags, smcmi_program **out, std::string *err, int32_t ens_para) {
    if (out) *out = nullptr;
    if (!source || !out) { *err = "smcmi_program_compile: null argument"; return SMCMI_ERR_ARG; }
    if (flags & ~(int32_t)SMCMI_PROGRAM_FUSED) { *err = "smcmi_program_compile_ex: unknown flag bits"; return SMCMI_ERR_ARG; }
    // an ENSEMBLE compile (ens_para != 0; flags are 0 then) is a fused compile with another kernel: the same options, refusals and named headers
    const bool ens = ens_para != 0;
    if (ens && (ens_para < enssrc::PARA_MIN || ens_para > enssrc::PARA_MAX)) { *err = "smcmi_program_compile_ensemble: n_para outside 1..10"; return SMCMI_ERR_ARG; }
    const bool fused = (flags & SMCMI_PROGRAM_FUSED) != 0, isolated = fused || ens;
    const char *ent = entry ? entry : progsrc::DEFAULT_ENTRY;
    if (!progsrc::valid_entry(ent)) { *err = "smcmi_program_compile: the entry is not a C identifier of at most 64 characters"; return SMCMI_ERR_ARG; }
    std::vector<std::string> extra;
    if (!progsrc::split_options(options, &extra, err)) return SMCMI_ERR_ARG;
    if (isolated && !fusedsrc::options_allowed(extra, err)) return SMCMI_ERR_ARG;
    if (!rtc_open(err)) return SMCMI_ERR_UNSUPPORTED;
    std::vector<std::string> opts = progsrc::base_options();
    if (isolated)
        for (const std::string &o : ens ? enssrc::extra_options() : fusedsrc::extra_options()) opts.push_back(o);
#ifdef SMCMI_STRICT_FP
    if (isolated) opts.push_back("-DSMCMI_STRICT_FP");           // (the embedded kernels.hpp: the same contraction rule as this library's own)
#endif
    opts.insert(opts.end(), extra.begin(), extra.end());
    std::vector<const char *> optv;
    for (const std::string &o : opts) optv.push_back(o.c_str());
    const progsrc::Assembled text = ens ? enssrc::assemble(source, ent, ens_para) : fused ? fusedsrc::assemble(source, ent) : progsrc::assemble(source, ent);
    // a fused or ensemble program reaches the project's device headers and the stand-ins of the system headers as named headers, and nothing else
    std::vector<const char *> hdr_text, hdr_name;
    if (isolated)
        for (const fusedsrc::Header &h : ens ? enssrc::header_table() : fusedsrc::header_table()) { hdr_name.push_back(h.name); hdr_text.push_back(h.text); }

    rtc_prog prog = nullptr;
    int rc = g_rtc.CreateProgram(&prog, text.text.c_str(), progsrc::USER_FILE, (int)hdr_name.size(), isolated ? hdr_text.data() : nullptr,
                                 isolated ? hdr_name.data() : nullptr);
    if (rc != 0 || !prog) { *err = "hiprtcCreateProgram: " + rtc_text(rc); return SMCMI_ERR_HIP; }
    smcmi_program *p = new smcmi_program();
    p->entry = ent;
    p->fused = fused;
    p->ens_para = ens_para;
    rc = g_rtc.CompileProgram(prog, (int)optv.size(), optv.data());
    size_t len = 0;
    if (g_rtc.GetProgramLogSize(prog, &len) == 0 && len > 1) {
        std::vector<char> buf(len + 1, '\0');
        if (g_rtc.GetProgramLog(prog, buf.data()) == 0) p->log = buf.data();
    }
    if (rc == 0) {
        size_t size = 0;
        rc = g_rtc.GetCodeSize(prog, &size);
        if (rc == 0 && size > 0) {
            p->code.resize(size);
            rc = g_rtc.GetCode(prog, p->code.data());
        }
        p->ok = rc == 0 && size > 0;
        // the code object's identity: FNV-1a over its bytes (smcmi_run_ensemble: do two members carry the same program?)
        p->id = 14695981039346656037ull;
        for (const char c : p->code) p->id = (p->id ^ (unsigned char)c) * 1099511628211ull;
        if (!p->ok && p->log.empty()) p->log = "the run-time compiler returned no code object: " + rtc_text(rc);
    } else if (p->log.empty()) p->log = rtc_text(rc);
    g_rtc.DestroyProgram(&prog);
    *out = p;
    if (!p->ok) {
        p->code.clear();
        *err = "the likelihood source did not compile (entry '" + p->entry + "'); smcmi_program_log has the compiler's messages";
        return SMCMI_ERR_COMPILE;
    }
    return SMCMI_OK;
}

int load(const smcmi_program *p, Loaded *out, std::string *err) {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    hipError_t e = hipModuleLoadData(&mod, p->code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&fn, mod, progsrc::KERNEL_NAME);
    hipFunction_t mut = nullptr;
    if (e == hipSuccess && p->fused) {
        e = hipModuleGetFunction(&mut, mod, fusedsrc::MUTATE_NAME);
        hipDeviceptr_t words = nullptr;
        size_t bytes = 0;
        if (e == hipSuccess) e = hipModuleGetGlobal(&words, &bytes, mod, fusedsrc::ABI_NAME);
        if (e == hipSuccess && bytes != sizeof(out->abi)) e = hipErrorInvalidImage;
        if (e == hipSuccess) e = hipMemcpyDtoH(out->abi, words, sizeof(out->abi));
    }
    hipFunction_t ensf = nullptr;
    if (e == hipSuccess && p->ens_para != 0) {
        e = hipModuleGetFunction(&ensf, mod, enssrc::ENSEMBLE_NAME);
        hipDeviceptr_t words = nullptr;
        size_t bytes = 0;
        if (e == hipSuccess) e = hipModuleGetGlobal(&words, &bytes, mod, enssrc::ABI_NAME);
        if (e == hipSuccess && bytes != sizeof(out->ens_abi)) e = hipErrorInvalidImage;
        if (e == hipSuccess) e = hipMemcpyDtoH(out->ens_abi, words, sizeof(out->ens_abi));
    }
    if (e != hipSuccess) {
        *err = std::string("loading the compiled likelihood: ") + hipGetErrorString(e);
        if (mod) (void)hipModuleUnload(mod);
        (void)hipGetLastError();
        return SMCMI_ERR_HIP;
    }
    out->module = (void *)mod;
    out->kernel = (void *)fn;
    out->mutate = (void *)mut;
    out->ensemble = (void *)ensf;
    out->ens_para = ensf ? p->ens_para : 0;
    out->id = p->id;
    return SMCMI_OK;
}
void unload(Loaded *l) {
    if (l->module) (void)hipModuleUnload((hipModule_t)l->module);
    l->module = nullptr;
    l->kernel = nullptr;
    l->mutate = nullptr;
    l->ensemble = nullptr;
    l->ens_para = 0;
    l->id = 0;
}

unsigned grid_for(long long n) {
    const long long nb = (n + progsrc::BLOCK - 1) / progsrc::BLOCK;
    return (unsigned)(nb < 1 ? 1 : nb > 2048 ? 2048 : nb);
}
int launch(const Loaded &l, const Args &a, void *stream) {
    Args v = a;
    void *args[] = {&v.theta, &v.gate, &v.n, &v.ld, &v.d, &v.data, &v.rows, &v.cols, &v.par, &v.n_par, &v.lik, &v.evals};
    return (int)hipModuleLaunchKernel((hipFunction_t)l.kernel, grid_for(a.n), 1, 1, progsrc::BLOCK, 1, 1, 0, (hipStream_t)stream, args, nullptr);
}
int launch_mutate(const Loaded &l, unsigned grid, unsigned block, size_t lds, void **args, void *stream) {
    // (more than 64 KiB of dynamic LDS: the runtime has no call that raises the maximum of a MODULE's function - hipFuncSetAttribute takes a
    // host function - and does not gate a module launch on it; the launch itself reports a request the device cannot serve)
    return (int)hipModuleLaunchKernel((hipFunction_t)l.mutate, grid, 1, 1, block, 1, 1, (unsigned)lds, (hipStream_t)stream, args, nullptr);
}

int launch_ensemble(const Loaded &l, unsigned grid, unsigned block, size_t lds, void **args, void *stream) {
    // (dynamic LDS above 64 KiB: as launch_mutate)
    return (int)hipModuleLaunchKernel((hipFunction_t)l.ensemble, grid, 1, 1, block, 1, 1, (unsigned)lds, (hipStream_t)stream, args, nullptr);
}

}      // namespace program
