// summary.hip - posterior summaries on the device (include/smcmi.h "posterior summaries"): weighted quantiles of parameter columns by
// selection (csrc/quantsel.hpp drives the passes, csrc/summary.hpp holds the kernels) and the best particle.  A translation unit of its
// own: nothing the engines' units compile depends on it.  One code path - the single-handle calls are the group of one; per pass the host
// reads every handle's sums and adds them in handle order.  The calls read the cloud and the device's buffer index, and write scratch memory
// that lives for the call only (from the handle's owner): nothing a later run depends on changes.
#define SMCMI_INST_UNIT 1               // (the engines' non-template kernels belong to smcmi.hip: kernels.hpp)
#include "handle.hpp"
#include "quantsel.hpp"
#include "summary.hpp"

namespace {

using summary::u64;

#define SUM_TRY(expr)                                         \
    do {                                                      \
        if ((expr) != hipSuccess) return SMCMI_ERR_HIP;      \
    } while (0)

// one handle's share of a call: where its cloud is, its launch geometry, its scratch memory (given back when the call returns)
struct Shard {
    smcmi_handle *h = nullptr;
    const double *cloud = nullptr;
    int nb = 1;
    char *base = nullptr;
    size_t cap = 0;
    int *d_cols = nullptr;
    u64 *d_thr = nullptr, *d_rec = nullptr, *d_keys = nullptr, *d_wmin = nullptr, *d_prev1 = nullptr, *d_bkey = nullptr;
    long long *d_bidx = nullptr;
    double *d_part = nullptr, *d_S = nullptr, *d_best = nullptr;
    std::vector<double> S;                   // host copies of what the passes leave
    std::vector<u64> rec, wmin, prev1;
    Shard() = default;
    Shard(const Shard &) = delete;
    Shard &operator=(const Shard &) = delete;
    ~Shard() {
        if (base && hipSetDevice(h->cfg.device) == hipSuccess) h->mem.release(&base);
    }
    int open(smcmi_handle *handle, int n_col) {
        h = handle;
        SUM_TRY(hipSetDevice(h->cfg.device));
        int cur = 0;
        SUM_TRY(hipMemcpyAsync(&cur, &h->d_st->cur, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        SUM_TRY(hipStreamSynchronize(h->stream));
        cloud = h->cl.buf[cur & 1];
        nb = summary::n_blocks(h->n);
        const size_t nc = (size_t)n_col;
        size_t off = 0;
        auto carve = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
        const size_t o_part = carve(nc * nb * summary::SLOTS * sizeof(double)), o_S = carve(nc * summary::SLOTS * sizeof(double)),
                     o_thr = carve(nc * summary::SLOTS * sizeof(u64)), o_rec = carve(nc * 4 * sizeof(u64)),
                     o_keys = carve(nc * summary::LEVELS * sizeof(u64)), o_wmin = carve(nc * summary::LEVELS * sizeof(u64)),
                     o_prev1 = carve(nc * summary::LEVELS * sizeof(u64)), o_cols = carve(nc * sizeof(int)),
                     o_bkey = carve((size_t)nb * sizeof(u64)), o_bidx = carve((size_t)nb * sizeof(long long)),
                     o_best = carve((size_t)(2 + h->d) * sizeof(double));
        SUM_TRY(h->mem.regrow(&base, &cap, off));
        d_part = (double *)(base + o_part); d_S = (double *)(base + o_S); d_thr = (u64 *)(base + o_thr); d_rec = (u64 *)(base + o_rec);
        d_keys = (u64 *)(base + o_keys); d_wmin = (u64 *)(base + o_wmin); d_prev1 = (u64 *)(base + o_prev1); d_cols = (int *)(base + o_cols);
        d_bkey = (u64 *)(base + o_bkey); d_bidx = (long long *)(base + o_bidx); d_best = (double *)(base + o_best);
        return 0;
    }
};

// the handles of one process that together hold one cloud, in rank order (uneven shards are fine: nothing here depends on their sizes)
int check_group(smcmi_handle **hs, int32_t n) {
    if (!hs || n < 1 || n > CENTER_SLOTS) return SMCMI_ERR_ARG;
    long long expect = 0;
    for (int k = 0; k < n; ++k) {
        if (!hs[k] || hs[k]->n < 1 || hs[k]->d != hs[0]->d || hs[k]->cfg.n_parts != hs[0]->cfg.n_parts || hs[k]->cfg.gid0 != expect) return SMCMI_ERR_ARG;
        expect += hs[k]->n;
    }
    return expect == hs[0]->cfg.n_parts ? 0 : SMCMI_ERR_ARG;
}

struct Group {
    std::vector<std::unique_ptr<Shard>> sh;
    std::vector<int> columns;                 // the requested cloud columns
    int wcol = 0;

    int open(smcmi_handle **hs, int n) {
        wcol = hs[0]->d + 4;
        for (int k = 0; k < n; ++k) {
            sh.emplace_back(new Shard());
            if (int e = sh.back()->open(hs[k], (int)columns.size())) return e;
        }
        return 0;
    }
    // the cloud columns behind positions `cols` of the request, to every handle
    std::vector<int> actual_cols(const std::vector<int> &cols) const {
        std::vector<int> actual(cols.size());
        for (size_t j = 0; j < cols.size(); ++j) actual[j] = columns[(size_t)cols[j]];
        return actual;
    }
    // (the source of an asynchronous copy stays as it is until the stream has been waited for: one vector for all handles)
    int upload_cols(Shard &s, const std::vector<int> &actual) {
        SUM_TRY(hipMemcpyAsync(s.d_cols, actual.data(), sizeof(int) * actual.size(), hipMemcpyHostToDevice, s.h->stream));
        return 0;
    }
    // S(t) for SLOTS thresholds per listed column: launched on every handle, then read and added in handle order
    int sums(const std::vector<int> &cols, const u64 *thr, double *S) {
        const size_t nc = cols.size(), m = nc * summary::SLOTS;
        const std::vector<int> actual = actual_cols(cols);
        for (auto &p : sh) {
            Shard &s = *p;
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            if (int e = upload_cols(s, actual)) return e;
            SUM_TRY(hipMemcpyAsync(s.d_thr, thr, sizeof(u64) * m, hipMemcpyHostToDevice, s.h->stream));
            summary::k_cand<<<dim3((unsigned)s.nb, (unsigned)nc), summary::TB, 0, s.h->stream>>>(s.cloud, s.h->n, wcol, s.d_cols, s.d_thr, s.d_part);
            summary::k_cand_final<<<(unsigned)nc, summary::TB, 0, s.h->stream>>>(s.d_part, s.nb, s.d_S);
            SUM_TRY(hipGetLastError());
            s.S.resize(m);
            SUM_TRY(hipMemcpyAsync(s.S.data(), s.d_S, sizeof(double) * m, hipMemcpyDeviceToHost, s.h->stream));
        }
        for (size_t r = 0; r < sh.size(); ++r) {
            Shard &s = *sh[r];
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            SUM_TRY(hipStreamSynchronize(s.h->stream));
            for (size_t j = 0; j < m; ++j) S[j] = r == 0 ? s.S[j] : S[j] + s.S[j];
        }
        return 0;
    }
    // smallest non-zero weight at LEVELS keys per listed column, and the largest key below each (+ 1; 0: none)
    int atkey(const std::vector<int> &cols, const u64 *keys, double *wmin, u64 *prev1) {
        const size_t nc = cols.size(), m = nc * summary::LEVELS;
        const std::vector<int> actual = actual_cols(cols);
        std::vector<u64> none(m, ~0ull);
        for (auto &p : sh) {
            Shard &s = *p;
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            if (int e = upload_cols(s, actual)) return e;
            SUM_TRY(hipMemcpyAsync(s.d_keys, keys, sizeof(u64) * m, hipMemcpyHostToDevice, s.h->stream));
            SUM_TRY(hipMemcpyAsync(s.d_wmin, none.data(), sizeof(u64) * m, hipMemcpyHostToDevice, s.h->stream));
            SUM_TRY(hipMemsetAsync(s.d_prev1, 0, sizeof(u64) * m, s.h->stream));
            summary::k_atkey<<<dim3((unsigned)s.nb, (unsigned)nc), summary::TB, 0, s.h->stream>>>(s.cloud, s.h->n, wcol, s.d_cols, s.d_keys, s.d_wmin, s.d_prev1);
            SUM_TRY(hipGetLastError());
            s.wmin.resize(m);
            s.prev1.resize(m);
            SUM_TRY(hipMemcpyAsync(s.wmin.data(), s.d_wmin, sizeof(u64) * m, hipMemcpyDeviceToHost, s.h->stream));
            SUM_TRY(hipMemcpyAsync(s.prev1.data(), s.d_prev1, sizeof(u64) * m, hipMemcpyDeviceToHost, s.h->stream));
        }
        std::vector<u64> wbits(m, ~0ull);
        for (size_t j = 0; j < m; ++j) prev1[j] = 0;
        for (auto &p : sh) {
            Shard &s = *p;
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            SUM_TRY(hipStreamSynchronize(s.h->stream));
            for (size_t j = 0; j < m; ++j) {
                wbits[j] = std::min(wbits[j], s.wmin[j]);
                prev1[j] = std::max(prev1[j], s.prev1[j]);
            }
        }
        for (size_t j = 0; j < m; ++j) {
            wmin[j] = 0.0;
            if (wbits[j] != ~0ull) std::memcpy(&wmin[j], &wbits[j], sizeof(double));
        }
        return 0;
    }
    // smallest / largest key and the flags of every requested column
    int minmax(std::vector<quantsel::Prepass> &pre, unsigned *flags_out) {
        const size_t nc = columns.size();
        const std::vector<int> &actual = columns;
        std::vector<u64> init(4 * nc, 0ull);
        for (size_t j = 0; j < nc; ++j) init[4 * j] = ~0ull;
        for (auto &p : sh) {
            Shard &s = *p;
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            if (int e = upload_cols(s, actual)) return e;
            SUM_TRY(hipMemcpyAsync(s.d_rec, init.data(), sizeof(u64) * 4 * nc, hipMemcpyHostToDevice, s.h->stream));
            summary::k_minmax<<<dim3((unsigned)s.nb, (unsigned)nc), summary::TB, 0, s.h->stream>>>(s.cloud, s.h->n, wcol, s.d_cols, s.d_rec);
            SUM_TRY(hipGetLastError());
            s.rec.resize(4 * nc);
            SUM_TRY(hipMemcpyAsync(s.rec.data(), s.d_rec, sizeof(u64) * 4 * nc, hipMemcpyDeviceToHost, s.h->stream));
        }
        unsigned flags = 0;
        for (size_t j = 0; j < nc; ++j) { pre[j].kmin = ~0ull; pre[j].kmax = 0ull; }
        for (auto &p : sh) {
            Shard &s = *p;
            SUM_TRY(hipSetDevice(s.h->cfg.device));
            SUM_TRY(hipStreamSynchronize(s.h->stream));
            for (size_t j = 0; j < nc; ++j) {
                pre[j].kmin = std::min(pre[j].kmin, (uint64_t)s.rec[4 * j]);
                pre[j].kmax = std::max(pre[j].kmax, (uint64_t)s.rec[4 * j + 1]);
                if (s.rec[4 * j + 2] & summary::FLAG_NAN_VALUE) pre[j].has_nan = true;
                flags |= (unsigned)s.rec[4 * j + 2];
            }
        }
        *flags_out = flags;
        return 0;
    }
};

int quantiles_impl(smcmi_handle **hs, int32_t n, const int32_t *columns, int32_t n_columns, const double *probs, int32_t n_probs, double *out) {
    if (int e = check_group(hs, n)) return e;
    if (!probs || !out || n_probs < 1 || n_probs > SMCMI_MAX_QUANT) return SMCMI_ERR_ARG;
    for (int q = 0; q < n_probs; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return SMCMI_ERR_ARG;
    const int d = hs[0]->d;
    Group g;
    if (!columns) {
        for (int j = 0; j < d; ++j) g.columns.push_back(j);
    } else {
        if (n_columns < 1 || n_columns > SMCMI_MAX_PARA) return SMCMI_ERR_ARG;
        for (int j = 0; j < n_columns; ++j) {
            if (columns[j] < 0 || columns[j] >= d) return SMCMI_ERR_ARG;
            g.columns.push_back(columns[j]);
        }
    }
    const int nc = (int)g.columns.size();
    if (int e = g.open(hs, n)) return e;
    // prepass: key range and flags of every column; w1 = the smallest weight at the smallest key; wsum out of the candidate pass's own tree
    std::vector<quantsel::Prepass> pre((size_t)nc);
    unsigned flags = 0;
    if (int e = g.minmax(pre, &flags)) return e;
    if ((flags & summary::FLAG_BAD_WEIGHT) || !(flags & summary::FLAG_SOME_WEIGHT)) return SMCMI_ERR_ARG;     // NaN / negative / infinite weight; all weights zero
    {
        std::vector<int> all((size_t)nc);
        std::vector<u64> keys((size_t)nc * summary::LEVELS, 0ull), prev1((size_t)nc * summary::LEVELS);
        std::vector<double> wmin((size_t)nc * summary::LEVELS);
        for (int j = 0; j < nc; ++j) { all[(size_t)j] = j; keys[(size_t)j * summary::LEVELS] = pre[(size_t)j].kmin; }
        if (int e = g.atkey(all, keys.data(), wmin.data(), prev1.data())) return e;
        for (int j = 0; j < nc; ++j) pre[(size_t)j].w1 = wmin[(size_t)j * summary::LEVELS];
        const std::vector<int> first(1, 0);
        std::vector<u64> thr(summary::SLOTS, ~0ull);
        std::vector<double> S(summary::SLOTS);
        if (int e = g.sums(first, thr.data(), S.data())) return e;
        if (!(S[0] > 0.0) || !(S[0] <= 1.7976931348623157e308)) return SMCMI_ERR_ARG;      // wsum == 0 (or not finite)
        for (int j = 0; j < nc; ++j) pre[(size_t)j].wsum = S[0];
    }
    return quantsel::select(
        nc, pre.data(), probs, n_probs, [&g](const std::vector<int> &cols, const uint64_t *thr, double *S) { return g.sums(cols, (const u64 *)thr, S); },
        [&g](const std::vector<int> &cols, const uint64_t *keys, double *wmin, uint64_t *prev1) { return g.atkey(cols, (const u64 *)keys, wmin, (u64 *)prev1); },
        out);
}

int best_impl(smcmi_handle **hs, int32_t n, int32_t criterion, int64_t *index_out, double *value_out, double *para_out) {
    if (int e = check_group(hs, n)) return e;
    if (criterion != SMCMI_BEST_LOGLH && criterion != SMCMI_BEST_LOGPOST) return SMCMI_ERR_ARG;
    const int d = hs[0]->d;
    Group g;
    g.columns.push_back(0);
    if (int e = g.open(hs, n)) return e;
    std::vector<std::vector<double>> best((size_t)n, std::vector<double>((size_t)d + 2));
    for (int r = 0; r < n; ++r) {
        Shard &s = *g.sh[(size_t)r];
        SUM_TRY(hipSetDevice(s.h->cfg.device));
        summary::k_best<<<(unsigned)s.nb, summary::TB, 0, s.h->stream>>>(s.cloud, s.h->n, d, criterion, s.d_bkey, s.d_bidx);
        summary::k_best_final<<<1, summary::TB, 0, s.h->stream>>>(s.cloud, s.h->n, d, criterion, s.d_bkey, s.d_bidx, s.nb, s.d_best);
        SUM_TRY(hipGetLastError());
        SUM_TRY(hipMemcpyAsync(best[(size_t)r].data(), s.d_best, sizeof(double) * ((size_t)d + 2), hipMemcpyDeviceToHost, s.h->stream));
    }
    int win = -1;
    u64 win_key = 0;
    for (int r = 0; r < n; ++r) {              // rank order = ascending global ids: only a strictly larger key replaces the winner
        Shard &s = *g.sh[(size_t)r];
        SUM_TRY(hipSetDevice(s.h->cfg.device));
        SUM_TRY(hipStreamSynchronize(s.h->stream));
        const double v = best[(size_t)r][1];
        const u64 key = v != v ? ~0ull : quantsel::key_of(v);
        if (win < 0 || key > win_key) { win = r; win_key = key; }
    }
    const std::vector<double> &b = best[(size_t)win];
    long long idx;
    std::memcpy(&idx, &b[0], sizeof idx);
    if (index_out) *index_out = (int64_t)(hs[win]->cfg.gid0 + idx);
    if (value_out) *value_out = b[1];
    if (para_out) std::memcpy(para_out, &b[2], sizeof(double) * (size_t)d);
    return 0;
}

}      // namespace

extern "C" int smcmi_weighted_quantiles_group(smcmi_handle **hs, int32_t n, const int32_t *columns, int32_t n_columns, const double *probs,
                                              int32_t n_probs, double *out) {
    return quantiles_impl(hs, n, columns, n_columns, probs, n_probs, out);
}
extern "C" int smcmi_weighted_quantiles(smcmi_handle *h, const int32_t *columns, int32_t n_columns, const double *probs, int32_t n_probs, double *out) {
    if (!h) return SMCMI_ERR_ARG;
    if (h->n != h->cfg.n_parts) return SMCMI_ERR_UNSUPPORTED;        // a lone shard: its group has the whole cloud
    return quantiles_impl(&h, 1, columns, n_columns, probs, n_probs, out);
}
extern "C" int smcmi_best_particle_group(smcmi_handle **hs, int32_t n, int32_t criterion, int64_t *index_out, double *value_out, double *para_out) {
    return best_impl(hs, n, criterion, index_out, value_out, para_out);
}
extern "C" int smcmi_best_particle(smcmi_handle *h, int32_t criterion, int64_t *index_out, double *value_out, double *para_out) {
    if (!h) return SMCMI_ERR_ARG;
    if (h->n != h->cfg.n_parts) return SMCMI_ERR_UNSUPPORTED;
    return best_impl(&h, 1, criterion, index_out, value_out, para_out);
}
