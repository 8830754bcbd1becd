// progsrc_check.cpp - csrc/progsrc.hpp on its own (host code, no HIP, no run-time compiler in this process): the text a run-time compiled
// likelihood is assembled into, the validation of the entry name, the splitting and the refusals of the caller's compiler options.
// Built by tests/test_program_cpu.py with -fsanitize=address,undefined; exit status 0 and nothing on stderr means every check held.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../smc.jl_amd/csrc/progsrc.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

// physical line (1-based) -> its text
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

static void check_assembly(const std::string &user, int expect_lines) {
    const progsrc::Assembled a = progsrc::assemble(user, "loglik");
    const std::vector<std::string> ls = lines_of(a.text);
    CHECK(a.user_lines == expect_lines);
    CHECK(a.user_first_line == 2);
    CHECK(a.wrapper_line_directive == 2 + expect_lines);
    CHECK(ls.size() > (size_t)a.wrapper_line_directive);
    CHECK(ls[0] == std::string("#line 1 \"") + progsrc::USER_FILE + "\"");
    // the wrapper's directive stands at the start of a line of its own, right behind the user's last line
    CHECK(ls[(size_t)a.wrapper_line_directive - 1] == std::string("#line 1 \"") + progsrc::WRAPPER_FILE + "\"");
    // every line of the user's text is line k of likelihood.hip, with the user's own characters
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
    // ... and the wrapper's first line is line 1 of its own file: no message about the wrapper is attributed to the user's text
    std::string file;
    int line = 0;
    logical(ls, a.wrapper_line_directive + 1, &file, &line);
    CHECK(file == progsrc::WRAPPER_FILE);
    CHECK(line == 1);
    CHECK(ls[(size_t)a.wrapper_line_directive].find("smcmi_program_kernel") != std::string::npos);
    CHECK(a.text.back() == '\n');
}

int main() {
    // ---- #line arithmetic, with and without a trailing newline
    check_assembly("", 0);
    check_assembly("double f();", 1);
    check_assembly("double f();\n", 1);
    check_assembly("a\nb\nc", 3);
    check_assembly("a\nb\nc\n", 3);
    check_assembly("\n\n", 2);
    check_assembly("a\n\n\nb", 4);
    {
        std::string big;
        for (int k = 0; k < 5000; ++k) big += "// line\n";
        check_assembly(big, 5000);
        check_assembly(big + "x", 5001);
    }
    // the entry's name reaches the wrapper's call, and only there
    {
        const progsrc::Assembled a = progsrc::assemble("", "my_lik_2");
        CHECK(a.text.find("v = my_lik_2(theta + i, ld, d, data, rows, cols, par, n_par);") != std::string::npos);
        CHECK(a.text.find("loglik") == std::string::npos);
    }

    // ---- entry validation
    CHECK(progsrc::valid_entry("loglik"));
    CHECK(progsrc::valid_entry("_x9"));
    CHECK(progsrc::valid_entry("L"));
    CHECK(!progsrc::valid_entry(nullptr));
    CHECK(!progsrc::valid_entry(""));
    CHECK(!progsrc::valid_entry("9x"));
    CHECK(!progsrc::valid_entry("a b"));
    CHECK(!progsrc::valid_entry(" a"));
    CHECK(!progsrc::valid_entry("a-b"));
    CHECK(!progsrc::valid_entry("a(b"));
    CHECK(!progsrc::valid_entry("caf\xc3\xa9"));
    CHECK(progsrc::valid_entry(std::string(64, 'a').c_str()));
    CHECK(!progsrc::valid_entry(std::string(65, 'a').c_str()));
    CHECK(!progsrc::valid_entry(std::string(100000, 'a').c_str()));

    // ---- option splitting
    std::vector<std::string> o;
    std::string why;
    CHECK(progsrc::split_options(nullptr, &o, &why) && o.empty());
    CHECK(progsrc::split_options("", &o, &why) && o.empty());
    CHECK(progsrc::split_options("   \t\n  ", &o, &why) && o.empty());
    CHECK(progsrc::split_options("-DNAME=3.5", &o, &why) && o.size() == 1 && o[0] == "-DNAME=3.5");
    CHECK(progsrc::split_options("  -DA=1\t-DB=2 \n -O2  ", &o, &why) && o.size() == 3 && o[0] == "-DA=1" && o[1] == "-DB=2" && o[2] == "-O2");
    {
        const std::string longopt = "-DX=" + std::string(200000, '1');
        CHECK(progsrc::split_options((longopt + " -DY=2").c_str(), &o, &why) && o.size() == 2 && o[0] == longopt && o[1] == "-DY=2");
        const std::string many = [] { std::string s; for (int k = 0; k < 3000; ++k) s += " -DZ" + std::to_string(k); return s; }();
        CHECK(progsrc::split_options(many.c_str(), &o, &why) && o.size() == 3000 && o[2999] == "-DZ2999");
    }
    // ---- refusals: whatever names a target, whatever contains xnack (either letter case, anywhere in the list)
    for (const char *bad : {"--offload-arch=gfx942", "-mcpu=gfx90a", "--offload-arch=gfx950:xnack+", "-mxnack", "-mno-xnack", "--OFFLOAD-ARCH=gfx950",
                            "-DA=1 -mcpu=gfx950", "-mcpu=gfx950 -DA=1", "\t-mXNACK\n", "-Xclang -target-feature -Xclang +xnack"}) {
        why.clear();
        o.assign(1, "stale");
        CHECK(!progsrc::split_options(bad, &o, &why));
        CHECK(o.empty());
        CHECK(!why.empty());
    }
    CHECK(!progsrc::split_options("-mxnack", &o, nullptr));          // (no room for the reason: still refused)
    // the library's own options: the target, and exact operations stay exact
    {
        const std::vector<std::string> b = progsrc::base_options();
        bool arch = false, contract = false;
        for (const std::string &s : b) { arch = arch || s == "--offload-arch=gfx950"; contract = contract || s == "-ffp-contract=off"; }
        CHECK(arch && contract);
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("progsrc_check ok\n");
    return 0;
}
