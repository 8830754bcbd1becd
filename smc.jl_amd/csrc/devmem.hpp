// devmem.hpp - who owns device and pinned memory.  The only place under csrc/ that calls the runtime's allocators and frees: a handle, an Eng2
// and each of the two callback buffer structs hold one Owner, which hands out raw pointers (kept where the launch sites read them) and gives
// back every buffer it made when it goes out of scope; a local Owner does the same for a call's temporary device words, Handles for the events
// and streams of a scope or a struct.  Depends on the HIP runtime API only, and the Owner takes its allocator through a policy, so a host-only
// program can drive it with a counting stand-in (tests/devmem_check.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <vector>

namespace devmem {

enum class Kind {
    Device,        // hipMalloc: coarse-grained device memory (the one kind SMCMI_POISON_ALLOC fills)
    FineGrained,   // device memory in which a peer GPU's stores and this GPU's polling loads meet (the mailbox tables)
    Pinned,        // page-locked host memory (staging buffers of the callback paths)
    Mapped         // page-locked host memory with a device alias (the note words a kernel posts to and the host polls)
};
static inline const char *kind_name(Kind k) {
    return k == Kind::Device ? "device" : k == Kind::FineGrained ? "fine-grained" : k == Kind::Pinned ? "pinned" : "mapped";
}

struct HipRuntime {
    static hipError_t allocate(void **p, size_t bytes, Kind k) {
        switch (k) {
        case Kind::Device: return hipMalloc(p, bytes);
        case Kind::FineGrained: return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained);
        case Kind::Pinned: return hipHostMalloc(p, bytes, hipHostMallocDefault);
        default: return hipHostMalloc(p, bytes, hipHostMallocMapped);
        }
    }
    static hipError_t device_alias(void **dev, void *host) { return hipHostGetDevicePointer(dev, host, 0); }
    static hipError_t release(void *p, Kind k) { return k == Kind::Device || k == Kind::FineGrained ? hipFree(p) : hipHostFree(p); }
    // (the fill runs on the null stream: it must not land after the first copies of a non-blocking stream)
    static hipError_t poison(void *p, size_t bytes) {
        const hipError_t e = hipMemset(p, 0xFF, bytes);
        return e != hipSuccess ? e : hipDeviceSynchronize();
    }
};

inline std::atomic<int> g_next_index{0};        // one numbering for every Owner of the process: a report line names one allocation

template <class Alloc = HipRuntime>
class Owner {
public:
    // development (SMCMI_POISON_ALLOC, set by whoever creates the owner): 1 = fresh device memory reads as NaN / -1, so a read of something never
    // written shows up in every test instead of depending on what the allocator hands back; 2 = every allocation and release is reported too
    int poison = 0;

    Owner() = default;
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    ~Owner() { release_all(); }

    // `count` elements (at least one) of kind `kind` into *p; Kind::Mapped also leaves the device alias in *alias.  On failure *p (and *alias)
    // are null and the owner holds nothing new.
    template <class T>
    hipError_t alloc(T **p, size_t count, Kind kind = Kind::Device, T **alias = nullptr) {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void *q = nullptr, *dq = nullptr;
        *p = nullptr;
        if (alias) *alias = nullptr;
        hipError_t e = Alloc::allocate(&q, bytes, kind);
        if (e != hipSuccess) return e;
        if (kind == Kind::Mapped) e = Alloc::device_alias(&dq, q);
        const bool fill = poison && kind == Kind::Device;
        if (e == hipSuccess && fill) e = Alloc::poison(q, bytes);
        if (e != hipSuccess) { (void)Alloc::release(q, kind); return e; }
        const int idx = g_next_index.fetch_add(1, std::memory_order_relaxed);
        held_.push_back({q, kind, idx});
        if (poison > 1) {
            if (fill) fprintf(stderr, "[smcmi] poisoned allocation #%d (%zu bytes)\n", idx, bytes);
            else fprintf(stderr, "[smcmi] allocation #%d (%zu bytes, %s)\n", idx, bytes, kind_name(kind));
        }
        *p = static_cast<T *>(q);
        if (alias) *alias = static_cast<T *>(dq);
        return hipSuccess;
    }
    // a buffer that only ever grows: released and allocated anew when `need` elements exceed *cap.  A failed allocation leaves it empty (*cap = 0).
    template <class T, class N>
    hipError_t regrow(T **p, N *cap, size_t need) {
        if ((size_t)*cap >= need) return hipSuccess;
        release(p);
        *cap = 0;
        const hipError_t e = alloc(p, need);
        if (e == hipSuccess) *cap = (N)need;
        return e;
    }
    // one buffer of this owner (a null *p: nothing to do)
    template <class T>
    void release(T **p) {
        if (!*p) return;
        for (size_t k = held_.size(); k-- > 0;)
            if (held_[k].p == (void *)*p) {
                give_back(held_[k]);
                held_.erase(held_.begin() + (long)k);
                break;
            }
        *p = nullptr;
    }
    void release_all() {
        for (size_t k = held_.size(); k-- > 0;) give_back(held_[k]);
        held_.clear();
    }
    size_t live() const { return held_.size(); }

private:
    struct Held { void *p; Kind kind; int idx; };
    std::vector<Held> held_;
    void give_back(const Held &h) {
        (void)Alloc::release(h.p, h.kind);
        if (poison > 1) fprintf(stderr, "[smcmi] released #%d\n", h.idx);
    }
};

// the events and streams made in a scope, or owned by a struct: destroyed with it, on every return
struct Handles {
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
    Handles() = default;
    Handles(const Handles &) = delete;
    Handles &operator=(const Handles &) = delete;
    ~Handles() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    }
    hipError_t event(hipEvent_t *e, unsigned flags = hipEventDefault) {
        const hipError_t r = hipEventCreateWithFlags(e, flags);
        if (r == hipSuccess) events.push_back(*e);
        return r;
    }
    hipError_t stream(hipStream_t *s, unsigned flags = hipStreamNonBlocking) {
        const hipError_t r = hipStreamCreateWithFlags(s, flags);
        if (r == hipSuccess) streams.push_back(*s);
        return r;
    }
};

}      // namespace devmem
