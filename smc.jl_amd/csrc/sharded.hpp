// sharded.hpp - the stage loop over particle shards (one shard per GPU), included by smcmi.hip.
//
// Replaces the reference's only parallel mode - `@distributed` over particles with the whole cloud serialised to every worker
// each stage (src/smc_main.jl:169-170, 472-476) - by resident shards and a handful of tiny in-stream collectives:
//   per solver pass : all-reduce of 2 KC doubles (Σv, Σv² per candidate)      correction : all-reduce of (ΣW̃, ΣW̃²)
//   moments         : all-reduce of 1 + d + d(d+1)/2 doubles                  mutation   : all-reduce of Σ accept
//   selection       : (ESS < threshold only) all-gather of the weight column and of the shard clouds; every rank forms the
//                     same global cumulative sum and gathers the ancestors of ITS output slots.
// The kernels are the single-GPU ones: a pass prologue / k_post_correct / k_prepare_mutation / k_stage_begin that is handed
// the all-reduced totals as "partials of 1 block" takes exactly the same decision on every rank.
// Two communicators implement the collectives: RCCL (one process per GPU, xGMI; the library is dlopen'ed so that libsmcmi.so
// has no hard dependency on it) and an in-process group of handles (single-process multi-shard runs; used by the GPU tests
// to exercise this driver with 2-4 shards on one device).
#pragma once
#include <dlfcn.h>

// ---- minimal RCCL surface (rccl.h:40-43 and the five entry points used), resolved at run time
struct smcmi_nccl_uid { char internal[128]; };
typedef void *smcmi_nccl_comm;
struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(smcmi_nccl_uid *) = nullptr;
    int (*CommInitRank)(smcmi_nccl_comm *, int, smcmi_nccl_uid, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, smcmi_nccl_comm, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, smcmi_nccl_comm, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, smcmi_nccl_comm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, smcmi_nccl_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommDestroy)(smcmi_nccl_comm) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
enum { SMCMI_NCCL_DOUBLE = 8, SMCMI_NCCL_SUM = 0 };   // ncclFloat64, ncclSum

static int load_rccl() {
    if (g_rccl.lib) return 0;
    const char *cands[] = {sw().rccl_path.c_str(), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *c : cands) {
        if (!c || !*c) continue;
        g_rccl.lib = dlopen(c, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return set_err(SMCMI_ERR_UNSUPPORTED, std::string("cannot load RCCL: ") + dlerror());
#define SMCMI_SYM(field, name) *(void **)(&g_rccl.field) = dlsym(g_rccl.lib, name)
    SMCMI_SYM(GetUniqueId, "ncclGetUniqueId"); SMCMI_SYM(CommInitRank, "ncclCommInitRank"); SMCMI_SYM(AllReduce, "ncclAllReduce");
    SMCMI_SYM(AllGather, "ncclAllGather"); SMCMI_SYM(Send, "ncclSend"); SMCMI_SYM(Recv, "ncclRecv");
    SMCMI_SYM(GroupStart, "ncclGroupStart"); SMCMI_SYM(GroupEnd, "ncclGroupEnd"); SMCMI_SYM(CommDestroy, "ncclCommDestroy"); SMCMI_SYM(GetErrorString, "ncclGetErrorString");
#undef SMCMI_SYM
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather)
        return set_err(SMCMI_ERR_UNSUPPORTED, "RCCL library lacks the required entry points");
    return 0;
}
#define NCCL_TRY(expr)                                                                                                    \
    do {                                                                                                                  \
        int r_ = (expr);                                                                                                  \
        if (r_ != 0) return set_err(SMCMI_ERR_HIP, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "nccl error")); \
    } while (0)

static void smcmi_comm_release(smcmi_handle *h) {
    if (h->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(h->nccl);
    h->nccl = nullptr;
}

extern "C" int smcmi_comm_unique_id(uint8_t *id_out) {
    if (!id_out) return set_err(SMCMI_ERR_ARG, "null argument");
    if (int rc = load_rccl()) return rc;
    smcmi_nccl_uid id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(id_out, id.internal, 128);
    return 0;
}

extern "C" int smcmi_comm_init(smcmi_handle *h, int32_t rank, int32_t world, const uint8_t *id) {
    if (!h || !id || world < 1 || rank < 0 || rank >= world) return set_err(SMCMI_ERR_ARG, "bad argument");
    if (h->cfg.n_local * world != h->cfg.n_parts || h->cfg.gid0 != rank * h->cfg.n_local)
        return set_err(SMCMI_ERR_ARG, "handle shard (n_local, gid0) does not match (rank, world): equal contiguous shards are required");
    if (int rc = load_rccl()) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    smcmi_nccl_uid uid;
    memcpy(uid.internal, id, 128);
    smcmi_nccl_comm c = nullptr;
    NCCL_TRY(g_rccl.CommInitRank(&c, world, uid, rank));
    h->nccl = c; h->rank = rank; h->world = world;
    h->has_hostc = false;                             // (a handle connected to a host communicator before: RCCL carries the collectives now)
    h->mbox_tried = false; h->mbox_ok = false;        // the peer tables of the previous communicator's ranks are not this one's
    // self-test: every rank contributes (1, rank) -> (world, world (world - 1) / 2); a broken transport fails here, loudly,
    // instead of producing a wrong posterior later
    if (!h->d_comm || h->comm_cap < 2) return set_err(SMCMI_ERR_STATE, "communication scratch buffer missing");
    const double mine[2] = {1.0, (double)rank};
    double got[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(h->d_comm, mine, sizeof(mine), hipMemcpyHostToDevice, h->stream));
    NCCL_TRY(g_rccl.AllReduce(h->d_comm, h->d_comm, 2, SMCMI_NCCL_DOUBLE, SMCMI_NCCL_SUM, h->nccl, h->stream));
    HIP_TRY(hipMemcpyAsync(got, h->d_comm, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (got[0] != (double)world || got[1] != 0.5 * (double)world * (double)(world - 1))
        return set_err(SMCMI_ERR_HIP, "RCCL all-reduce self-test failed (got " + std::to_string(got[0]) + ", " + std::to_string(got[1]) + ")");
    return 0;
}

// ---- host-mediated communicator (include/smcmi.h smcmi_host_comm): the same collectives carried by caller-supplied functions on host
// buffers - for ranks that share a GPU or have no RCCL (the multi-process tests on one GPU, bring-up behind MPI / gloo / Distributed.jl).
// Every collective is: stream sync -> device-to-host -> callback -> host-to-device on the handle's stream -> sync, so kernels enqueued
// behind it see its result exactly as they see an in-stream RCCL collective's.
extern "C" int smcmi_comm_init_host(smcmi_handle *h, int32_t rank, int32_t world, const smcmi_host_comm *comm) {
    if (!h || !comm || !comm->allgather || !comm->barrier || world < 1 || rank < 0 || rank >= world) return set_err(SMCMI_ERR_ARG, "bad argument");
    if (h->cfg.n_local * world != h->cfg.n_parts || h->cfg.gid0 != rank * h->cfg.n_local)
        return set_err(SMCMI_ERR_ARG, "handle shard (n_local, gid0) does not match (rank, world): equal contiguous shards are required");
    if (h->nccl) smcmi_comm_release(h);
    h->has_hostc = false;
    h->mbox_tried = false; h->mbox_ok = false;
    // self-test, as smcmi_comm_init: every rank contributes (1, rank); the handle counts as connected only once it has passed
    const double mine[2] = {1.0, (double)rank};
    std::vector<double> all(2 * (size_t)world, 0.0);
    if (comm->allgather(mine, all.data(), 2, comm->user)) return set_err(SMCMI_ERR_CALLBACK, "host communicator: allgather failed");
    for (int r = 0; r < world; ++r)
        if (all[2 * r] != 1.0 || all[2 * r + 1] != (double)r) return set_err(SMCMI_ERR_CALLBACK, "host communicator: allgather self-test failed (rank order?)");
    h->hostc = *comm; h->has_hostc = true; h->rank = rank; h->world = world;
    return 0;
}
static int hostc_allgather(smcmi_handle *h, const double *dsend, double *drecv, size_t count) {
    std::vector<double> &sb = h->hc_send, &rb = h->hc_recv;
    sb.resize(count); rb.resize(count * (size_t)h->world);
    HIP_TRY(hipMemcpyAsync(sb.data(), dsend, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->hostc.allgather(sb.data(), rb.data(), (int64_t)count, h->hostc.user)) return set_err(SMCMI_ERR_CALLBACK, "host communicator: allgather failed");
    if (!drecv) return 0;                  // (the caller reads h->hc_recv on the host)
    HIP_TRY(hipMemcpyAsync(drecv, rb.data(), sizeof(double) * rb.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

constexpr int MAX_SHARDS = 64;     // slots for the per-shard energy maxima behind the all-reduced epilogue row
static inline int shard_rank(const smcmi_handle *h) { return (int)(h->cfg.gid0 / h->cfg.n_local); }

// ---- collectives over a group of lock-stepped local handles, optionally extended over ranks by RCCL
struct ShardGroup {
    std::vector<smcmi_handle *> hs;   // local shards (same process); RCCL mode: exactly one
    int world = 1;                    // total number of shards
    bool rccl = false;                // one local handle, the other shards in other processes ("remote")
    bool hostc = false;               // remote through the handle's host-mediated communicator instead of RCCL

    int sync_all() {
        for (auto *h : hs) { HIP_TRY(hipSetDevice(h->cfg.device)); HIP_TRY(hipStreamSynchronize(h->stream)); }
        return 0;
    }
    // in-place sum of `count` doubles at buf(h) over all shards, same result everywhere (fixed shard order)
    template <class F>
    int allreduce(F buf, int count) {
        if (rccl && hostc) {          // all-gather, then the sum in rank order (the same bits on every rank)
            smcmi_handle *h = hs[0];
            if (int rc = hostc_allgather(h, buf(h), nullptr, (size_t)count)) return rc;      // gathered on the host: h->hc_recv
            std::vector<double> tot(count, 0.0);
            for (int r = 0; r < world; ++r)
                for (int k = 0; k < count; ++k) tot[k] += h->hc_recv[(size_t)r * count + k];
            HIP_TRY(hipMemcpyAsync(buf(h), tot.data(), sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            return 0;
        }
        if (rccl) {
            smcmi_handle *h = hs[0];
            NCCL_TRY(g_rccl.AllReduce(buf(h), buf(h), (size_t)count, SMCMI_NCCL_DOUBLE, SMCMI_NCCL_SUM, h->nccl, h->stream));
            return 0;
        }
        if (hs.size() == 1) return 0;
        if (int rc = sync_all()) return rc;
        std::vector<double> tot(count, 0.0), tmp(count);
        for (auto *h : hs) {
            HIP_TRY(hipSetDevice(h->cfg.device));
            HIP_TRY(hipMemcpy(tmp.data(), buf(h), sizeof(double) * count, hipMemcpyDeviceToHost));
            for (int k = 0; k < count; ++k) tot[k] += tmp[k];
        }
        for (auto *h : hs) {
            HIP_TRY(hipSetDevice(h->cfg.device));
            HIP_TRY(hipMemcpy(buf(h), tot.data(), sizeof(double) * count, hipMemcpyHostToDevice));
        }
        return 0;
    }
    // every handle's stream has reached this point before any goes on (RCCL: an in-stream all-reduce of one double)
    int barrier() {
        if (rccl && hostc) {
            smcmi_handle *h = hs[0];
            HIP_TRY(hipStreamSynchronize(h->stream));
            if (h->hostc.barrier(h->hostc.user)) return set_err(SMCMI_ERR_CALLBACK, "host communicator: barrier failed");
            return 0;
        }
        if (rccl) {
            smcmi_handle *h = hs[0];
            NCCL_TRY(g_rccl.AllReduce(h->d_comm, h->d_comm, (size_t)1, SMCMI_NCCL_DOUBLE, SMCMI_NCCL_SUM, h->nccl, h->stream));
            return 0;
        }
        return sync_all();
    }
    // recv(h)[r * count .. (r+1) * count) = send(shard r)
    template <class FS, class FR>
    int allgather(FS send, FR recv, size_t count) {
        if (rccl && hostc) return hostc_allgather(hs[0], send(hs[0]), recv(hs[0]), count);
        if (rccl) {
            smcmi_handle *h = hs[0];
            NCCL_TRY(g_rccl.AllGather(send(h), recv(h), count, SMCMI_NCCL_DOUBLE, h->nccl, h->stream));
            return 0;
        }
        // (the copies go on the DESTINATION handle's stream, behind which its consumers are enqueued: the handles' streams are
        // non-blocking, a device-to-device hipMemcpy on the null stream is ordered with none of them and need not have finished when
        // it returns - consumers could read the table before the copy landed, and once in a few hundred runs did)
        if (int rc = sync_all()) return rc;
        for (auto *dst : hs) {
            HIP_TRY(hipSetDevice(dst->cfg.device));
            for (size_t r = 0; r < hs.size(); ++r)
                HIP_TRY(hipMemcpyAsync(recv(dst) + r * count, send(hs[r]), sizeof(double) * count, hipMemcpyDeviceToDevice, dst->stream));
        }
        return sync_all();                     // (and no source may go on before every copy out of it is done)
    }
    // Resample redistribution as an all-to-all-v (systematic resampling: the ancestors of a shard's output slots form one
    // contiguous global row range [lo[r], hi[r]]).  Every shard receives exactly the rows of that range, column by column, into
    // the [source shard][column][row] staging layout the all-gather would have produced, so k_resample_gather is unchanged.
    // ranges = (lo, hi) per shard, identical on every shard (all derive it from the same all-gathered cumulative weights).
    // with_cum: the rows' values of the handle's cum column (d_cum, local index) travel as one more column into d_cum_full (global index)
    int exchange_rows(const std::vector<long long> &ranges, bool with_cum = false) {
        const long long n = hs[0]->n;
        const int R = hs[0]->R;
        auto overlap = [&](int needer, int owner, long long &a, long long &b) {     // rows of `owner` that `needer` needs: [a, b)
            a = std::max(ranges[2 * needer], (long long)owner * n);
            b = std::min(ranges[2 * needer + 1] + 1, (long long)(owner + 1) * n);
            return b > a;
        };
        if (rccl && hostc) {
            // all-to-all-v on host buffers: per peer one [R][rows] block, packed from / unpacked into the column-major device layouts
            smcmi_handle *h = hs[0];
            const int me = h->rank;
            if (!h->hostc.alltoallv) return set_err(SMCMI_ERR_UNSUPPORTED, "host communicator lacks alltoallv (SMCMI_RESAMPLE_EXCHANGE=allgather avoids it)");
            const int RC = R + (with_cum ? 1 : 0);              // columns per row on the wire
            std::vector<int64_t> sc(world, 0), sd(world, 0), rcnt(world, 0), rd(world, 0);
            std::vector<long long> sa(world, 0), ra(world, 0);
            int64_t stot = 0, rtot = 0;
            for (int p = 0; p < world; ++p) {
                long long a, b;
                if (p != me && overlap(p, me, a, b)) { sc[p] = (b - a) * RC; sa[p] = a - (long long)me * n; }
                if (p != me && overlap(me, p, a, b)) { rcnt[p] = (b - a) * RC; ra[p] = a - (long long)p * n; }
                sd[p] = stot; stot += sc[p];
                rd[p] = rtot; rtot += rcnt[p];
            }
            std::vector<double> sbuf((size_t)std::max<int64_t>(stot, 1)), rbuf((size_t)std::max<int64_t>(rtot, 1));
            for (int p = 0; p < world; ++p)
                if (sc[p]) {
                    const long long len = sc[p] / RC;
                    HIP_TRY(hipMemcpy2DAsync(sbuf.data() + sd[p], sizeof(double) * len, h->cl.buf[0] + sa[p], sizeof(double) * n, sizeof(double) * (size_t)len, (size_t)R,
                                             hipMemcpyDeviceToHost, h->stream));
                    if (with_cum) HIP_TRY(hipMemcpyAsync(sbuf.data() + sd[p] + (size_t)R * len, h->d_cum + sa[p], sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, h->stream));
                }
            HIP_TRY(hipStreamSynchronize(h->stream));
            if (h->hostc.alltoallv(sbuf.data(), sc.data(), sd.data(), rbuf.data(), rcnt.data(), rd.data(), h->hostc.user))
                return set_err(SMCMI_ERR_CALLBACK, "host communicator: alltoallv failed");
            for (int p = 0; p < world; ++p)
                if (rcnt[p]) {
                    const long long len = rcnt[p] / RC;
                    HIP_TRY(hipMemcpy2DAsync(h->d_full_cloud + (long long)p * R * n + ra[p], sizeof(double) * n, rbuf.data() + rd[p], sizeof(double) * len, sizeof(double) * (size_t)len,
                                             (size_t)R, hipMemcpyHostToDevice, h->stream));
                    if (with_cum) HIP_TRY(hipMemcpyAsync(h->d_cum_full + (long long)p * n + ra[p], rbuf.data() + rd[p] + (size_t)R * len, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, h->stream));
                }
            long long a, b;
            if (overlap(me, me, a, b)) {
                HIP_TRY(hipMemcpy2DAsync(h->d_full_cloud + (long long)me * R * n + (a - (long long)me * n), sizeof(double) * n,
                                         h->cl.buf[0] + (a - (long long)me * n), sizeof(double) * n, sizeof(double) * (size_t)(b - a), (size_t)R,
                                         hipMemcpyDeviceToDevice, h->stream));
                if (with_cum) HIP_TRY(hipMemcpyAsync(h->d_cum_full + a, h->d_cum + (a - (long long)me * n), sizeof(double) * (size_t)(b - a), hipMemcpyDeviceToDevice, h->stream));
            }
            HIP_TRY(hipStreamSynchronize(h->stream));
            return 0;
        }
        if (rccl) {
            smcmi_handle *h = hs[0];
            const int me = h->rank;
            if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
                return set_err(SMCMI_ERR_UNSUPPORTED, "RCCL library lacks send/recv");
            NCCL_TRY(g_rccl.GroupStart());
            for (int p = 0; p < world; ++p) {
                long long a, b;
                if (overlap(p, me, a, b) && p != me) {                                 // my rows that p needs
                    for (int c = 0; c < R; ++c)
                        NCCL_TRY(g_rccl.Send(h->cl.buf[0] + (long long)c * n + (a - (long long)me * n), (size_t)(b - a), SMCMI_NCCL_DOUBLE, p, h->nccl, h->stream));
                    if (with_cum) NCCL_TRY(g_rccl.Send(h->d_cum + (a - (long long)me * n), (size_t)(b - a), SMCMI_NCCL_DOUBLE, p, h->nccl, h->stream));
                }
                if (overlap(me, p, a, b) && p != me) {                                 // p's rows that I need
                    for (int c = 0; c < R; ++c)
                        NCCL_TRY(g_rccl.Recv(h->d_full_cloud + ((long long)p * R + c) * n + (a - (long long)p * n), (size_t)(b - a), SMCMI_NCCL_DOUBLE, p, h->nccl, h->stream));
                    if (with_cum) NCCL_TRY(g_rccl.Recv(h->d_cum_full + a, (size_t)(b - a), SMCMI_NCCL_DOUBLE, p, h->nccl, h->stream));
                }
            }
            NCCL_TRY(g_rccl.GroupEnd());
            long long a, b;
            if (overlap(me, me, a, b)) {
                HIP_TRY(hipMemcpy2DAsync(h->d_full_cloud + (long long)me * R * n + (a - (long long)me * n), sizeof(double) * n,
                                         h->cl.buf[0] + (a - (long long)me * n), sizeof(double) * n, sizeof(double) * (size_t)(b - a), (size_t)R,
                                         hipMemcpyDeviceToDevice, h->stream));
                if (with_cum) HIP_TRY(hipMemcpyAsync(h->d_cum_full + a, h->d_cum + (a - (long long)me * n), sizeof(double) * (size_t)(b - a), hipMemcpyDeviceToDevice, h->stream));
            }
            return 0;
        }
        if (int rc = sync_all()) return rc;
        for (size_t d = 0; d < hs.size(); ++d)
            for (size_t o = 0; o < hs.size(); ++o) {
                long long a, b;
                if (!overlap((int)d, (int)o, a, b)) continue;
                HIP_TRY(hipSetDevice(hs[d]->cfg.device));
                HIP_TRY(hipMemcpy2DAsync(hs[d]->d_full_cloud + (long long)o * R * n + (a - (long long)o * n), sizeof(double) * n,
                                         hs[o]->cl.buf[0] + (a - (long long)o * n), sizeof(double) * n, sizeof(double) * (size_t)(b - a), (size_t)R,
                                         hipMemcpyDeviceToDevice, hs[d]->stream));
                if (with_cum) HIP_TRY(hipMemcpyAsync(hs[d]->d_cum_full + a, hs[o]->d_cum + (a - (long long)o * n), sizeof(double) * (size_t)(b - a), hipMemcpyDeviceToDevice, hs[d]->stream));
            }
        return sync_all();
    }
};

static int ensure_shard_buffers(smcmi_handle *h) {
    const long long N = h->cfg.n_parts;
    if (!h->d_tot_ess) {
        if (dmalloc(h->mem, &h->d_tot_ess, 2 * KC) || dmalloc(h->mem, &h->d_tot_fin, 2) || dmalloc(h->mem, &h->d_tot_mom, h->npairs + 2) || dmalloc(h->mem, &h->d_tot_acc, ES + MAX_SHARDS))
            return SMCMI_ERR_HIP;
        HIP_TRY(hipMemsetAsync(h->d_tot_acc, 0, sizeof(double) * (ES + MAX_SHARDS), h->stream));   // (the handle's stream is non-blocking: keep its work on it)
    }
    if (!h->d_cum_full) {
        if (dmalloc(h->mem, &h->d_cum_full, N)) return SMCMI_ERR_HIP;
        h->nb_full = (int)std::min<long long>(1024, std::max<long long>(1, (N + 511) / 512));
        if (dmalloc(h->mem, &h->d_part_full, (size_t)h->nb_full * 2) || dmalloc(h->mem, &h->d_off_full, h->nb_full)) return SMCMI_ERR_HIP;
    }
    if (!h->d_full_w) {
        if (dmalloc(h->mem, &h->d_full_w, N) || dmalloc(h->mem, &h->d_full_cloud, (size_t)N * h->R)) return SMCMI_ERR_HIP;
    }
    return 0;
}


// The shift of a chain's first moments over all shards (smcmi.hip center_probe): every shard's row of column minima / maxima, gathered by the
// sum all-reduce, the same shift on every shard.  The shards' "my cloud came from outside" words travel with the rows, so every rank takes
// the same decision on a continuation without knowing the others' history; the caller enqueues center_apply behind the push of each
// handle's DevState.
static_assert(MAX_SHARDS <= CENTER_SLOTS, "one centre row per shard");
static int center_group(ShardGroup &g, bool fresh) {
    if (!center_on()) return 0;
    const int d = g.hs[0]->d;
    if (!fresh) {
        // a continuation: the shards' "my cloud came from outside" words first - in-process shards are all here; ranks sum theirs - and
        // nothing more when no cloud did (stage-at-a-time drivers continue once per stage)
        bool any = false;
        for (auto *h : g.hs) any = any || h->center_stale;
        if (g.rccl) {
            static const double word[2] = {0.0, 1.0};
            smcmi_handle *h = g.hs[0];
            HIP_TRY(hipSetDevice(h->cfg.device));
            HIP_TRY(hipMemcpyAsync(center_rows(h), &word[any ? 1 : 0], sizeof(double), hipMemcpyHostToDevice, h->stream));
            if (int rc2 = g.allreduce([](smcmi_handle *q) { return center_rows(q); }, 1)) return rc2;
            double sum = 0.0;
            HIP_TRY(hipMemcpyAsync(&sum, center_rows(h), sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            any = sum > 0.0;
        }
        if (!any) {                              // center_apply's word: nothing to take
            for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); HIP_TRY(hipMemsetAsync(center_out(h) + d, 0, sizeof(double), h->stream)); }
            return 0;
        }
        // (the clouds came through smcmi_upload_cloud and its kin, which pull the state: h_st.cur below is the device's)
    }
    for (auto *h : g.hs) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rank = g.world > 1 ? (g.rccl ? h->rank : shard_rank(h)) : 0;
        if (int e = center_probe(h, rank, g.world)) return e;
    }
    const int count = g.world * (2 * d + 1);
    if (g.world > 1) { if (int rc2 = g.allreduce([](smcmi_handle *h) { return center_rows(h); }, count)) return rc2; }
    for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); center_shift(h, g.world, fresh); }
    return 0;
}

// one stage, phase by phase over all local shards (the phases between collectives are independent per shard)
static int run_sharded_impl(ShardGroup &g, const smcmi_run_config *rc, smcmi_result *res) {
    smcmi_handle *h0 = g.hs[0];
    for (auto *h : g.hs) { if (int e = check_run_config(h, rc)) return e; }
    const bool adaptive = !rc->use_fixed_schedule;
    const int P_default = adaptive ? (rc->solver_passes >= 1 ? rc->solver_passes : SHARDED_SOLVER_PASSES) : 0;
    // User likelihoods on the host (the reference's default use: smc(loglikelihood::Function, ...) with parallel = true, src/smc_main.jl:118,
    // 472-476): every shard scores the proposals of ITS particles through its registered callback (callback.hpp host_mutation: propose
    // kernel -> closure on the calling thread -> accept kernel), everything else - solver passes, correction, selection, moments,
    // proposal set-up, the collectives - is this driver's.  The callback mutation leaves neither energy sums nor energy maxima, so
    // such runs walk the schedule without a predictor, unshifted, one stage per host sync (the closure needs the host anyway).
    // (a device callback - smcmi_set_likelihood_device - takes the same route: host_mutation branches on the kind)
    const bool host_mut = closure_lik(h0), tempered_cb = closure_lik(h0, 1), dev_cb = device_lik(h0);
    for (auto *h : g.hs)
        if (closure_lik(h) != host_mut || closure_lik(h, 1) != tempered_cb || device_lik(h) != dev_cb) return set_err(SMCMI_ERR_STATE, "every shard needs the same likelihood callbacks");
    const bool predict = adaptive && !sw().no_predictor && !host_mut;
    const int sel_mode = sw().no_select_predict;   // development only
    const bool predict_select = adaptive && can_fuse_post(h0) && sel_mode != 1 && !host_mut;
    const std::vector<double> sched = make_schedule(rc);
    for (auto *h : g.hs) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        if (ensure_shard_buffers(h) || pull_state(h) || upload_sched(h, sched.data(), rc->n_phi)) return SMCMI_ERR_HIP;
        if (host_mut) { if (int e = dev_cb ? ensure_dev_callback_buffers(h) : ensure_callback_buffers(h)) return e; h->rng_ahead = false; h->cb_energy = false; h->cb_calls = 0; h->cb_evals = 0; if (int e = prog_reset(h)) return e; }
        else if (int e = ensure_zbuf(h, rc->n_mh_steps, rc->n_blocks)) return e;
        // (a continuation: every shard keeps the loop scalars, records and history it holds - the same scalars on every shard)
        if (int e = start_state(h, rc, make_run_params(h, rc), false)) return e;
        if (rc->continue_run) { if (h->h_st.stage != h0->h_st.stage) return set_err(SMCMI_ERR_STATE, "shards hold different loop states"); }
        else if (int e = first_records(h, rc)) return e;
    }
    if (g.world > MAX_SHARDS) return set_err(SMCMI_ERR_ARG, "too many shards");
    if (int e = center_group(g, !rc->continue_run)) return e;
    for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); center_apply(h); }
    // stage 1's energy shift: largest energy of the initial cloud over all shards (slots after the ES row: a sum all-reduce
    // in which every shard fills only its own slot is a gather)
    if (!host_mut) {
    for (auto *h : g.hs) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int nb0 = mut_blocks(h);
        k_energy_max<<<nb0, TB, 0, h->stream>>>(h->cl, h->d_st, h->d_emax_part);
        k_reduce_partials<<<1, TB, 0, h->stream>>>(nullptr, 0, 0, nullptr, h->d_emax_part, nb0, h->d_tot_acc + ES, shard_rank(h), g.world);
    }
    if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_acc + ES; }, g.world)) return rc2;
    } else {                                  // stage 2's begin folds "the last acceptance rate": none yet
        for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); HIP_TRY(hipMemsetAsync(h->d_tot_acc, 0, sizeof(double) * (ES + MAX_SHARDS), h->stream)); }
    }
    // One stage = the single-GPU launch sequence with the collectives in-stream.  Nothing in it needs the host: on an adaptive
    // schedule the selection path - all-gather of weights and shard clouds, global scan, gather - is enqueued exactly where a
    // resample is forecast (stagepolicy.hpp; its kernels gate themselves on the device's decision) and elsewhere k_moments_reg
    // takes the post-correction decision itself; a wrong expectation or a solver that runs out of passes stalls the run
    // (done = 3 / 2) identically on every rank and is resumed at the next host sync.  Fixed schedules cannot be predicted: they
    // keep one flag read per stage.
    // use_graph == 2: HIP events around the first local shard's mutation launches (the `roofline` figure of a multi-GPU bench line)
    MutationEvents evs(rc->use_graph == 2);
    // the global cumulative weights on every shard, from the all-gathered weight column
    auto scan_full = [&](smcmi_handle *h) {
        CloudPtrs wcl{};
        wcl.buf[0] = wcl.buf[1] = h->d_full_w; wcl.n = h->cfg.n_parts; wcl.R = 1;
        k_weight_chunk_sums<<<h->nb_full, TB, 0, h->stream>>>(wcl, h->d_st, h->d_part_full);
        k_chunk_offsets<<<1, 1, 0, h->stream>>>(h->d_st, h->d_part_full, h->nb_full, h->d_off_full, 0.0, 0);
        k_scan_weights<<<h->nb_full, TB, 0, h->stream>>>(wcl, h->d_st, h->d_off_full, h->d_cum_full, 0, h->nb_full);
    };
    auto gather_full = [&](smcmi_handle *h) {
        const long long N = h->cfg.n_parts;
        k_resample_gather<<<(unsigned)((h->n + TB - 1) / TB), TB, 0, h->stream>>>(h->cl, h->d_st, h->d_cum_full, N, h->cfg.gid0, N, rc->resampling_method,
                                                                                h->cfg.seed, 0u, nullptr, h->d_anc, h->d_full_cloud, 0, h->n, 1, h->d_full_w);
    };
    // proposal set-up from the all-reduced moments, the mutation, and what the next begin reads of it totalled over all shards
    auto mutate_and_reduce = [&](int prep_mode, int fin_slot) -> int {
        for (auto *h : g.hs) {
            HIP_TRY(hipSetDevice(h->cfg.device));
            launch_prepare_in_run(h, h->d_tot_mom, 1, prep_mode, fin_slot);
            hipEvent_t pe0 = nullptr, pe1 = nullptr;
            if (h == h0) { evs.pair(0, &pe0, &pe1); if (pe0) hipEventRecord(pe0, h->stream); }
            const int nbl = launch_mutate(h, rc->n_blocks, 0, rc->alpha);
            if (pe1) hipEventRecord(pe1, h->stream);
            if (predict) k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_esum_part, nbl, ES, h->d_tot_acc, h->d_emax_part, nbl, h->d_tot_acc + ES, shard_rank(h), g.world);
            else k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_acc_part, nbl, 1, h->d_tot_acc + EACC, h->d_emax_part, nbl, h->d_tot_acc + ES, shard_rank(h), g.world);
        }
        if (predict) return g.allreduce([](smcmi_handle *h) { return h->d_tot_acc; }, ES + g.world);
        return g.allreduce([](smcmi_handle *h) { return h->d_tot_acc + EACC; }, 1 + g.world);
    };
    // q (run1.hpp StageReq): passes p0 .. p0 + passes - 1; spec: no certificate pass, no all-reduce for it - 2 collectives per stage
    auto enqueue = [&](const StageReq &q) -> int {
        const int p0 = q.p0, P = q.spec ? 0 : p0 + q.passes;
        const int fin_slot = P == 0 ? 0 : (P & 1);
        // no selection expected + register kernels: the correction pass gathers the moments too, so (ΣW̃, ΣW̃², pair sums) travel
        // in ONE all-reduce (3 collectives per stage instead of 4); k_prepare_mutation decides, the mutation kernel normalises
        const bool cm = q.no_select && can_fuse_cm(h0);
        const int npf = h0->npairs + 2;
        for (auto *h : g.hs) { h->fused_cm = cm; h->spec_stage = q.spec && cm; }
        if (q.tail_only) {
            // resume of a stalled stage: its correction left the per-block (ΣW̃, ΣW̃²) partials - total them first
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_part_fin, h->nb_e, 2, h->d_tot_fin);
            }
            if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_fin; }, 2)) return rc2;
        }
        if (!q.tail_only) {
            if (p0 == 0 && !q.skip_begin)
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    h->run_adaptive = predict;
                    k_stage_begin<<<1, BT, 0, h->stream>>>(h->d_st, h->d_sched, h->d_tot_acc + EACC, 1, h->rec, predict ? h->d_tot_acc : nullptr, nullptr,
                                                   h->spec_stage ? 1 : 0, host_mut ? nullptr : h->d_tot_acc + ES, g.world);
                }
            for (int p = p0; p < P; ++p) {
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    k_pass<KC, false><<<h->nb_e, TB, 0, h->stream>>>(h->cl, h->d_st, h->d_sched, h->d_tot_ess, h->d_part_ess[p & 1], 1, p, nullptr, 0);
                    k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_part_ess[p & 1], h->nb_e, 2 * KC, h->d_tot_ess);
                }
                if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_ess; }, 2 * KC)) return rc2;
            }
            if (cm) {
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    launch_correct_moments(h, P, h->d_tot_ess, 1);
                    k_moments_reduce<<<(npf + 63) / 64, 1024, 0, h->stream>>>(h->d_st, h->d_part_cm, h->nb_e, npf, h->d_tot_mom, 0);
                }
                if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_mom; }, npf)) return rc2;
            } else {
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    k_pass<1, true><<<h->nb_e, TB, 0, h->stream>>>(h->cl, h->d_st, h->d_sched, h->d_tot_ess, h->d_part_fin, 1, P, h->d_hist_w, h->n);
                    k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_part_fin, h->nb_e, 2, h->d_tot_fin);
                }
                if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_fin; }, 2)) return rc2;
            }
        }
        if (cm) return mutate_and_reduce(3, fin_slot);
        if (q.no_select) {
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                // the moments kernel decides from the all-reduced (ΣW̃, ΣW̃²) handed over as the partials of one block
                switch (h->d) {
#define SMCMI_FUSED_CASE(D) case D: k_moments_reg<D><<<h->nb_mr, TB, 0, h->stream>>>(h->cl, h->d_st, h->d_part_mom, h->d_hist_W, h->n, 0, h->d_tot_fin, 1, fin_slot, h->rec); break;
                SMCMI_FUSED_CASE(1) SMCMI_FUSED_CASE(2) SMCMI_FUSED_CASE(3) SMCMI_FUSED_CASE(4) SMCMI_FUSED_CASE(5) SMCMI_FUSED_CASE(6)
                SMCMI_FUSED_CASE(7) SMCMI_FUSED_CASE(8) SMCMI_FUSED_CASE(9) SMCMI_FUSED_CASE(10) SMCMI_FUSED_CASE(11) SMCMI_FUSED_CASE(12)
#undef SMCMI_FUSED_CASE
                default: return set_err(SMCMI_ERR_STATE, "fused post-correction needs d <= 12");
                }
                k_moments_reduce<<<(h->npairs + 63) / 64, 1024, 0, h->stream>>>(h->d_st, h->d_part_mom, h->nb_mr, h->npairs, h->d_tot_mom, 0);
            }
        } else {
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                k_post_correct<<<1, TB, 0, h->stream>>>(h->d_st, h->d_tot_fin, 1, nullptr, h->rec, fin_slot);
            }
            int rs = 1;
            if (!adaptive || !predict_select) {
                // the one host decision per stage of the unpredicted path (identical on all ranks)
                int fl[2] = {0, 0};
                HIP_TRY(hipSetDevice(h0->cfg.device));
                HIP_TRY(hipMemcpyAsync(&fl[0], &h0->d_st->do_resample, sizeof(int), hipMemcpyDeviceToHost, h0->stream));
                HIP_TRY(hipMemcpyAsync(&fl[1], &h0->d_st->done, sizeof(int), hipMemcpyDeviceToHost, h0->stream));
                HIP_TRY(hipStreamSynchronize(h0->stream));
                rs = fl[0] && !fl[1];
            }
            // resample redistribution: all-to-all-v of exactly the rows each shard's slots descend from (systematic resampling; the
            // default), or an all-gather of the whole cloud (multinomial resampling, or SMCMI_RESAMPLE_EXCHANGE=allgather)
            const bool a2a = rs && !sw().resample_allgather && rc->resampling_method == SMCMI_RESAMPLE_SYSTEMATIC && g.world > 1;
            const size_t nloc = (size_t)h0->n;
            if (rs) {                                      // either way the weights are all-gathered (N doubles)
                if (int rc2 = g.allgather([](smcmi_handle *h) { return (const double *)(h->cl.buf[0] + (long long)(h->R - 1) * h->n); },
                                          [](smcmi_handle *h) { return h->d_full_w; }, nloc)) return rc2;
            }
            if (a2a) {
                // all-to-all-v redistribution: every shard forms the global cumulative sum and the ancestor range of every shard's slots;
                // then only the rows inside a shard's range travel to it
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    scan_full(h);
                    k_anc_ranges<<<1, 64, 0, h->stream>>>(h->d_st, h->d_cum_full, h->cfg.n_parts, h->n, g.world, h->cfg.seed, h->d_anc, h->d_full_w);
                }
                std::vector<long long> ranges(2 * (size_t)g.world);
                HIP_TRY(hipSetDevice(h0->cfg.device));
                HIP_TRY(hipMemcpyAsync(ranges.data(), h0->d_anc, sizeof(long long) * ranges.size(), hipMemcpyDeviceToHost, h0->stream));
                HIP_TRY(hipStreamSynchronize(h0->stream));
                if (ranges[0] >= 0) {                      // -1: the device decided not to resample after all
                    if (int rc2 = g.exchange_rows(ranges)) return rc2;
                    for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); gather_full(h); }
                }
            } else if (rs) {
                if (int rc2 = g.allgather([](smcmi_handle *h) { return (const double *)h->cl.buf[0]; },
                                          [](smcmi_handle *h) { return h->d_full_cloud; }, nloc * h0->R)) return rc2;
                for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); scan_full(h); gather_full(h); }
            }
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                const int nbm = launch_moments(h, h->d_hist_W, 0);
                k_moments_reduce<<<(h->npairs + 63) / 64, 1024, 0, h->stream>>>(h->d_st, h->d_part_mom, nbm, h->npairs, h->d_tot_mom, 0);
            }
        }
        if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_mom; }, h0->npairs)) return rc2;
        if (host_mut) {
            // the closure scores every shard's proposals; a stage that did not run on the device (stall, pause, ϕ = 1 reached, error - the
            // same on every rank: all decisions come from all-reduced totals) must not reach it
            for (auto *h : g.hs) { HIP_TRY(hipSetDevice(h->cfg.device)); launch_prepare_in_run(h, h->d_tot_mom, 1, 2); }
            int dn = 0;
            HIP_TRY(hipSetDevice(h0->cfg.device));
            HIP_TRY(hipMemcpyAsync(&dn, &h0->d_st->done, sizeof(int), hipMemcpyDeviceToHost, h0->stream));
            HIP_TRY(hipStreamSynchronize(h0->stream));
            if (dn) return 0;
            // (a closure that fails on ONE rank must end the stage on every rank: the failure rides the acceptance all-reduce as a second
            // number - a rank that returned alone would leave the others waiting in the collective)
            int my_err = 0;
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                const int e = my_err ? my_err : host_mutation(h, rc, tempered_cb);
                if (e) my_err = e;
                else k_reduce_partials<<<1, TB, 0, h->stream>>>(h->d_acc_part, h->nb_mut, 1, h->d_tot_acc + EACC);
                const double flag = e ? 1.0 : 0.0;
                HIP_TRY(hipMemcpyAsync(h->d_tot_acc + EACC + 1, &flag, sizeof(double), hipMemcpyHostToDevice, h->stream));
                HIP_TRY(hipStreamSynchronize(h->stream));           // (`flag` is a stack variable)
            }
            const std::string my_msg = my_err ? g_err : std::string();
            if (int rc2 = g.allreduce([](smcmi_handle *h) { return h->d_tot_acc + EACC; }, 2)) return rc2;
            double failed = 0.0;
            HIP_TRY(hipSetDevice(h0->cfg.device));
            HIP_TRY(hipMemcpyAsync(&failed, h0->d_tot_acc + EACC + 1, sizeof(double), hipMemcpyDeviceToHost, h0->stream));
            HIP_TRY(hipStreamSynchronize(h0->stream));
            if (my_err) return set_err(my_err, my_msg);
            if (failed != 0.0) return set_err(SMCMI_ERR_CALLBACK, "the likelihood callback failed on another rank of the sharded run");
            return 0;
        }
        return mutate_and_reduce(2, 0);
    };

    const auto t0 = std::chrono::steady_clock::now();
    const bool cont = rc->continue_run != 0;
    const int base = cont ? h0->h_st.stage - 1 : 0;      // stages completed before this call
    const int max_iter = (adaptive ? h0->cfg.max_stages : rc->n_phi - 1) - base;
    const int sync_every = rc->sync_every > 0 ? rc->sync_every : 16;
    const double N_tot = (double)h0->cfg.n_parts;
    stagepolicy::Forecast forecast(rc->tempering_target, N_tot, rc->threshold_ratio * N_tot, cont ? h0->h_st.ess_prev : (rc->initial_ess > 0.0 ? rc->initial_ess : N_tot),
                                   cont ? h0->h_st.resampled_last : 0);
    int done = 0, iters = 0;
    const bool spec_ok = predict_select && predict && can_fuse_cm(h0) &&
                         rc->tempered_update_prior_weight == 0.0 && !(rc->phi_rtol < 0.0);
    stagepolicy::StallBook book(std::max(P_default, FIRST_SOLVER_PASSES), P_default, 4, base, spec_ok);
    stagepolicy::StagesLeft left;
    while (iters < max_iter && !done) {
        const int batch = host_mut ? 1 : (adaptive ? left.batch(sync_every, max_iter - iters) : max_iter - iters);
        for (int b = 0; b < batch; ++b) {
            StageReq q;
            if (predict_select) q.no_select = !forecast.step() || sel_mode == 2;
            q.spec = book.spec_on && q.no_select && iters >= 2;
            q.passes = adaptive ? book.fresh(iters) : 0;
            if (int rc2 = enqueue(q)) return rc2;
            ++iters;
        }
        // one 64-byte copy per sync: done flag, resample flag and ESS of the last stage are contiguous in DevState
        DevState head;
        constexpr size_t head_off = offsetof(DevState, stage), head_len = offsetof(DevState, ess) - offsetof(DevState, stage);
        for (;;) {
            HIP_TRY(hipSetDevice(h0->cfg.device));
            HIP_TRY(hipMemcpyAsync((char *)&head + head_off, (const char *)h0->d_st + head_off, head_len, hipMemcpyDeviceToHost, h0->stream));
            HIP_TRY(hipStreamSynchronize(h0->stream));
            done = head.done;
            if (done != 2 && done != 3 && done != 4) break;
            // stall (identical on every rank: all decisions come from all-reduced totals): clear it and resume that stage
            if (pull_state(h0)) return SMCMI_ERR_HIP;
            const int st_i = h0->h_st.stage;
            for (auto *h : g.hs) {
                HIP_TRY(hipSetDevice(h->cfg.device));
                const int zero = 0;
                HIP_TRY(hipMemcpyAsync(&h->d_st->done, &zero, sizeof(int), hipMemcpyHostToDevice, h->stream));
            }
            if (done == 4)
                for (auto *h : g.hs) {
                    HIP_TRY(hipSetDevice(h->cfg.device));
                    k_solver_rearm<<<1, 64, 0, h->stream>>>(h->d_st, h->d_sched);
                }
            StageReq q;
            if (!resume_request(book, done, st_i, &q)) return bracket_error();
            if (int rc2 = enqueue(q)) return rc2;
            iters = st_i - 1 - base;
        }
        if (!done && head.phi_n >= 1.0) break;      // the last stage of the batch reached ϕ = 1: the closing k_stage_begin finishes
        left.observe(head.phi_n, head.phi_n - head.phi_prev);
        if (predict_select) forecast.anchor(head.ess_prev, head.resampled_last);    // (the copy that ended the loop above)
    }
    // fold the last acceptance rate, close the run
    for (auto *h : g.hs) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        k_stage_begin<<<1, BT, 0, h->stream>>>(h->d_st, h->d_sched, h->d_tot_acc + EACC, 1, h->rec);
        if (pull_state(h)) return SMCMI_ERR_HIP;
        if (int e = prog_collect(h)) return e;
        h->last_n_stages = h->h_st.stage;
    }
    const auto t1 = std::chrono::steady_clock::now();
    const DevState &s = h0->h_st;
    memset(res, 0, sizeof(*res));
    finish_result(res, s, t0, t1);
    put_stalls(res, book);
    // (launches of stalled - no-op - stages are short and rare: they stay in the mean)
    if (int e = evs.tally(h0, 1, res)) return e;
    return finish_error(s);
}
