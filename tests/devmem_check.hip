// devmem_check.hip - fault injection into csrc/devmem.hpp's Owner.  Host code only, no device needed:
//     hipcc --offload-arch=gfx950 --offload-host-only -O1 -std=c++17 -Xarch_host -fsanitize=address,undefined tests/devmem_check.hip -o devmem_check
// The owner runs on a counting allocator (malloc / free behind the policy's interface) that fails on its k-th call and aborts on a release of a
// pointer it does not hold.  Three scripted sequences - one shaped like smcmi_create, a regrow whose allocation fails after the release, a
// scoped temporary with an early return - run for every k from 1 to the sequence's length and once without a failure: after the owner has
// gone out of scope nothing is live, nothing was released twice, and the indices the owner reported as released are the ones it reported
// as allocated.  tests/test_abi_cpu.py builds and runs it: exit status 0, nothing on stderr.
#include "../smc.jl_amd/csrc/devmem.hpp"

#include <unistd.h>

#include <cstdlib>
#include <cstring>
#include <set>

using devmem::Kind;

struct Counting {
    static inline int calls = 0, fail_at = 0;
    static inline std::set<void *> live;
    static bool fails() { return ++calls == fail_at; }
    static hipError_t allocate(void **p, size_t bytes, Kind) {
        if (fails()) return hipErrorOutOfMemory;
        *p = malloc(bytes);
        live.insert(*p);
        return hipSuccess;
    }
    static hipError_t device_alias(void **dev, void *host) {
        if (fails()) return hipErrorInvalidValue;
        *dev = host;
        return hipSuccess;
    }
    static hipError_t release(void *p, Kind) {
        if (!live.erase(p)) {
            fprintf(stdout, "release of %p, which the allocator does not hold\n", p);
            abort();
        }
        free(p);
        return hipSuccess;
    }
    static hipError_t poison(void *p, size_t bytes) {
        if (fails()) return hipErrorInvalidValue;
        memset(p, 0xFF, bytes);
        return hipSuccess;
    }
};
using Owner = devmem::Owner<Counting>;

// ---- the three sequences; each returns 0 or the error its first failing step gave
struct Handle {                     // (the shape of smcmi_handle: raw pointers where the launch sites read them, the owner last)
    double *cloud[2] = {nullptr, nullptr}, *rec[5] = {}, *scratch[28] = {};
    unsigned long long *mbox = nullptr;
    double *staging[2] = {nullptr, nullptr};
    int *h_note = nullptr, *d_note = nullptr;
    Owner mem;
};
#define TRY(expr) do { if ((expr) != hipSuccess) return 1; } while (0)
static int create_like(Handle *h, bool later_step_fails) {
    h->mem.poison = 2;
    for (double *&p : h->cloud) TRY(h->mem.alloc(&p, 4096 * 8));
    for (double *&p : h->rec) TRY(h->mem.alloc(&p, 100));
    for (int k = 0; k < 28; ++k) TRY(h->mem.alloc(&h->scratch[k], (size_t)(k % 3 ? 64 * k : 0)));      // (0: one element)
    TRY(h->mem.alloc(&h->mbox, 1024, Kind::FineGrained));
    for (double *&p : h->staging) TRY(h->mem.alloc(&p, 512, Kind::Pinned));
    TRY(h->mem.alloc(&h->h_note, 16, Kind::Mapped, &h->d_note));
    if (h->d_note != h->h_note) return 2;
    h->mem.release(&h->rec[2]);                            // (smcmi_set_likelihood: one buffer goes and comes back)
    if (h->rec[2]) return 2;
    TRY(h->mem.alloc(&h->rec[2], 200));
    if (later_step_fails) return 1;                        // (a push or a hipFuncSetAttribute behind the allocations)
    return 0;
}
static int run_create(bool later_step_fails) {
    Handle *h = new Handle();
    const int rc = create_like(h, later_step_fails);
    delete h;                                              // (smcmi_create's one exit, and smcmi_destroy)
    return rc;
}
static int run_regrow(bool) {
    Owner o;
    o.poison = 2;
    double *p = nullptr;
    size_t cap = 0;
    int *q = nullptr, qcap = 0;
    TRY(o.regrow(&q, &qcap, 7));
    for (size_t need : {10, 5, 100, 50, 1000}) {
        const double *before = p;
        const size_t cap0 = cap;
        if (o.regrow(&p, &cap, need) != hipSuccess) {
            if (p || cap) return 2;                        // released, not allocated: empty, and the owner no longer holds the old buffer
            if (o.live() != 1) return 2;
            TRY(o.regrow(&p, &cap, need));                 // ... and the next call allocates
            if (!p || cap != need) return 2;
            return 1;
        }
        if (need <= cap0 && (p != before || cap != cap0)) return 2;
        if (need > cap0 && cap != need) return 2;
        p[need - 1] = 1.0;
    }
    return 0;
}
static int temporary(bool early) {
    Owner tmp;
    tmp.poison = 2;
    int *d_send = nullptr, *d_recv = nullptr;
    TRY(tmp.alloc(&d_send, 8));
    if (early) return 1;
    TRY(tmp.alloc(&d_recv, 64));
    return 0;
}

// ---- one run of a sequence with the k-th allocator call failing (0: none); the owner's report is read back from stderr
static int failures = 0;
static void fail(const char *seq, int k, const char *what) { printf("%s, k = %d: %s\n", seq, k, what); ++failures; }
static int run_one(const char *seq, int (*fn)(bool), bool flag, int k) {
    FILE *cap = tmpfile();
    fflush(stderr);
    const int saved = dup(2);
    dup2(fileno(cap), 2);
    Counting::calls = 0; Counting::fail_at = k; Counting::live.clear();
    const int rc = fn(flag);
    fflush(stderr);
    dup2(saved, 2);
    close(saved);
    const int calls = Counting::calls;
    if (rc == 2) fail(seq, k, "the sequence saw a state it must not see");
    if ((rc != 0) != (flag || (k >= 1 && k <= calls))) fail(seq, k, "the injected failure was not returned");
    if (!Counting::live.empty()) fail(seq, k, "allocations are live after the owner went out of scope");
    std::multiset<int> made, gone;
    char line[256];
    rewind(cap);
    while (fgets(line, sizeof line, cap)) {
        int idx = -1;
        if (sscanf(line, "[smcmi] poisoned allocation #%d", &idx) == 1 || sscanf(line, "[smcmi] allocation #%d", &idx) == 1) made.insert(idx);
        else if (sscanf(line, "[smcmi] released #%d", &idx) == 1) gone.insert(idx);
        else fail(seq, k, line);
    }
    fclose(cap);
    if (made != gone) fail(seq, k, "released indices differ from allocated indices");
    if (std::set<int>(made.begin(), made.end()).size() != made.size()) fail(seq, k, "an index was given twice");
    for (void *p : Counting::live) free(p);
    return calls;
}
static void run_all(const char *seq, int (*fn)(bool), bool flag, int min_calls) {
    const int len = run_one(seq, fn, flag, 0);
    if (len < min_calls) fail(seq, 0, "the sequence is shorter than scripted");
    for (int k = 1; k <= len; ++k) run_one(seq, fn, flag, k);
}

int main() {
    run_all("create", run_create, false, 2 * 36 + 1 + 2 + 2);      // (device allocations are two calls each: allocate, poison)
    run_all("create, a later step fails", run_create, true, 2 * 36 + 1 + 2 + 2);
    run_all("regrow", run_regrow, false, 2 * 4);
    run_all("temporary", temporary, false, 4);
    run_all("temporary, early return", temporary, true, 2);
    if (failures) printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
