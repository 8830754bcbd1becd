// enssrc_check.cpp - csrc/enssrc.hpp on its own (host code, no HIP, no run-time compiler in this process): the translation unit a likelihood
// compiled FOR ENSEMBLES is assembled into, and the table of named headers it is compiled against.
// Built by tests/test_program_ensemble_cpu.py with -fsanitize=address,undefined and -I <the build directory that holds embedded_headers.inc
// and embedded_ens_headers.inc>; argv[1] is csrc.  Exit status 0 and nothing on stderr means every check held.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../smc.jl_amd/csrc/enssrc.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static std::vector<std::string> lines_of(const std::string &t) {
    std::vector<std::string> out;
    std::string cur;
    for (char c : t) {
        if (c == '\n') { out.push_back(cur); cur.clear(); }
        else cur += c;
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

// what a compiler following the #line directives calls physical line `phys`: (file, line)
static void logical(const std::vector<std::string> &ls, int phys, std::string *file, int *line) {
    *file = "<input>";
    int cur = 0;
    for (int k = 1; k <= phys; ++k) {
        ++cur;
        const std::string &s = ls[(size_t)k - 1];
        if (k == phys) break;
        int n = 0;
        char name[128];
        if (sscanf(s.c_str(), "#line %d \"%127[^\"]\"", &n, name) == 2) { cur = n - 1; *file = name; }
    }
    *line = cur;
}

static void check_assembly(const std::string &user, int expect_lines, int n_para) {
    const progsrc::Assembled a = enssrc::assemble(user, "loglik", n_para);
    const std::vector<std::string> ls = lines_of(a.text);
    CHECK(a.user_lines == expect_lines);
    CHECK(a.user_first_line == 2);
    CHECK(a.wrapper_line_directive == 2 + expect_lines);
    CHECK(ls.size() > (size_t)a.wrapper_line_directive + 4);
    CHECK(ls[0] == std::string("#line 1 \"") + progsrc::USER_FILE + "\"");
    CHECK(ls[(size_t)a.wrapper_line_directive - 1] == std::string("#line 1 \"") + progsrc::WRAPPER_FILE + "\"");
    const std::vector<std::string> ul = lines_of(user);
    CHECK((int)ul.size() == expect_lines);
    for (int k = 1; k <= expect_lines; ++k) {
        std::string file;
        int line = 0;
        logical(ls, a.user_first_line + k - 1, &file, &line);
        CHECK(file == progsrc::USER_FILE);
        CHECK(line == k);
        CHECK(ls[(size_t)(a.user_first_line + k - 2)] == ul[(size_t)k - 1]);
    }
    // behind the user's text, in this order: the defines, the include of ensbody.hpp, the wrapper kernel, the ensemble kernel, the ABI words
    std::string file;
    int line = 0;
    logical(ls, a.wrapper_line_directive + 1, &file, &line);
    CHECK(file == progsrc::WRAPPER_FILE && line == 1);
    CHECK(ls[(size_t)a.wrapper_line_directive] == "#define SMCMI_PROGRAM_ENTRY ::loglik");
    const size_t p_def = a.text.find("#define SMCMI_PROGRAM_ENTRY"), p_ens = a.text.find("#define SMCMI_PROGRAM_ENS 1"),
                 p_inc = a.text.find("#include \"ensbody.hpp\""), p_wrap = a.text.find("smcmi_program_kernel("),
                 p_kern = a.text.find("smcmi_program_ensemble("), p_abi = a.text.find("smcmi_program_ens_abi[4]");
    CHECK(p_def != std::string::npos && p_ens != std::string::npos && p_inc != std::string::npos && p_wrap != std::string::npos &&
          p_kern != std::string::npos && p_abi != std::string::npos);
    CHECK(p_def < p_ens && p_ens < p_inc && p_inc < p_wrap && p_wrap < p_kern && p_kern < p_abi);
    CHECK(a.text.find("smcmi::ens_run_body<" + std::to_string(n_para) + ">(a, progs);") != std::string::npos);
    // the wrapper kernel is the split path's, character for character, and the fused kernel is not part of this unit
    CHECK(a.text.find(progsrc::wrapper_text("loglik")) != std::string::npos);
    CHECK(a.text.find(fusedsrc::MUTATE_NAME) == std::string::npos);
    CHECK(a.text.back() == '\n');
}

// the names of the #include lines of `text`: "name" -> quoted, <name> -> angled
static void includes_of(const std::string &text, std::set<std::string> *quoted, std::set<std::string> *angled) {
    for (const std::string &l : lines_of(text)) {
        size_t p = l.find_first_not_of(" \t");
        if (p == std::string::npos || l[p] != '#') continue;
        p = l.find_first_not_of(" \t", p + 1);
        if (p == std::string::npos || l.compare(p, 7, "include") != 0) continue;
        p = l.find_first_of("\"<", p + 7);
        if (p == std::string::npos) continue;
        const char close = l[p] == '"' ? '"' : '>';
        const size_t q = l.find(close, p + 1);
        if (q == std::string::npos) continue;
        (close == '"' ? quoted : angled)->insert(l.substr(p + 1, q - p - 1));
    }
}

int main(int argc, char **argv) {
    // ---- #line arithmetic, with and without a trailing newline, for the smallest and the largest n_para
    for (int d : {enssrc::PARA_MIN, 3, enssrc::PARA_MAX}) {
        check_assembly("", 0, d);
        check_assembly("double f();", 1, d);
        check_assembly("double f();\n", 1, d);
        check_assembly("a\nb\nc", 3, d);
        check_assembly("a\nb\nc\n", 3, d);
        check_assembly("\n\n", 2, d);
        check_assembly("a\n\n\nb", 4, d);
    }
    {
        std::string big;
        for (int k = 0; k < 5000; ++k) big += "// line\n";
        check_assembly(big, 5000, 10);
        check_assembly(big + "x", 5001, 10);
    }
    CHECK(enssrc::PARA_MIN == 1 && enssrc::PARA_MAX == 10);
    // the entry's name reaches the define and the wrapper's call
    {
        const progsrc::Assembled a = enssrc::assemble("", "my_lik_2", 7);
        CHECK(a.text.find("#define SMCMI_PROGRAM_ENTRY ::my_lik_2\n") != std::string::npos);
        CHECK(a.text.find("v = my_lik_2(theta + i, ld, d, data, rows, cols, par, n_par);") != std::string::npos);
        CHECK(a.text.find("loglik") == std::string::npos);
        CHECK(a.text.find("ens_run_body<7>") != std::string::npos);
    }

    // ---- the options: the system include paths are off; the refusals are a fused compile's (fusedsrc::options_allowed, checked there)
    {
        bool nostdinc = false, nostdincxx = false;
        for (const std::string &o : enssrc::extra_options()) { nostdinc = nostdinc || o == "-nostdinc"; nostdincxx = nostdincxx || o == "-nostdinc++"; }
        CHECK(nostdinc && nostdincxx);
        std::string why;
        CHECK(!fusedsrc::options_allowed({"-DSMCMI_PROGRAM_ENS=0"}, &why));
    }

    // ---- the header table: unique names, the fused compile's headers and the two the ensemble kernel adds, and every header an #include of the
    // embedded text names is in it
    const std::vector<fusedsrc::Header> table = enssrc::header_table();
    std::set<std::string> names;
    for (const fusedsrc::Header &h : table) {
        CHECK(h.name && h.text && *h.name);
        CHECK(names.insert(h.name).second);
    }
    CHECK(table.size() == fusedsrc::header_table().size() + 2);
    CHECK(enssrc::ensemble_headers().size() == 2);
    CHECK(names.count(enssrc::BODY_HEADER) == 1 && names.count("ensshape.hpp") == 1 && names.count(fusedsrc::KERNELS_HEADER) == 1);
    std::vector<fusedsrc::Header> project = fusedsrc::project_headers();
    project.insert(project.end(), enssrc::ensemble_headers().begin(), enssrc::ensemble_headers().end());
    for (const fusedsrc::Header &h : project) {
        std::set<std::string> quoted, angled;
        includes_of(h.text, &quoted, &angled);
        for (const std::string &n : quoted) {
            if (names.count(n) != 1) { printf("FAILED: %s includes \"%s\", which the header table lacks\n", h.name, n.c_str()); ++g_fail; }
        }
        for (const std::string &n : angled) {
            if (names.count(n) != 1) { printf("FAILED: %s includes <%s>, which the header table lacks\n", h.name, n.c_str()); ++g_fail; }
        }
    }
    // ---- the embedded text is the files' text, byte for byte (argv[1] = csrc)
    CHECK(argc == 2);
    if (argc == 2) {
        for (const fusedsrc::Header &h : enssrc::ensemble_headers()) {
            std::ifstream f(std::string(argv[1]) + "/" + h.name, std::ios::binary);
            CHECK(f.good());
            std::stringstream ss;
            ss << f.rdbuf();
            if (ss.str() != h.text) { printf("FAILED: the embedded %s differs from the file\n", h.name); ++g_fail; }
            CHECK(!ss.str().empty());
        }
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("enssrc_check ok\n");
    return 0;
}
