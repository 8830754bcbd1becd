// devcallback.hpp - the USER likelihood as a device function (included by callback.hpp, main translation unit only).
//
// smcmi_set_likelihood_device registers a function that receives DEVICE pointers and the handle's stream (include/smcmi.h): a torch
// function, or a HIP kernel of the user's own.  The propose / accept split of the host-callback path stays (k_mutate<1> -> likelihood ->
// k_mutate<2>), but nothing crosses PCIe: the engine's share of the path - keeping out-of-bounds proposals away from the user's function
// (the reference never calls the likelihood after a ParamBoundsError, mutation.jl:93), NaN -> -Inf (its try / catch), the redraw loop of
// the initial draw (initialization.jl:23-63) - runs in the kernels below, on the handle's stream.  The only thing the host reads per MH
// step x block is the number of in-bounds proposals (8 bytes): the user's function needs the shape.
#pragma once

struct DevCallbackBuffers {
    long long n = 0;
    int d = 0;
    double *d_pack = nullptr;        // m x d in-bounds proposals, column-major with leading dimension m (only when m < n)
    double *d_out = nullptr;         // the user's function's m results of a packed batch
    long long *d_pos = nullptr;      // row i -> its position in the packed batch, -1: the bounds check failed
    long long *d_blk = nullptr;      // per-block counts of in-bounds rows, then their exclusive prefix sums
    long long *d_cnt = nullptr;      // [0] m of the last count, [1] rows the initial draw has to redraw
    long long *h_cnt = nullptr;      // pinned: where the host reads them
    long long m = 0;                 // of the last count (the old-data callback of a tempered update scores the same batch)
    double phase_ms[CBP_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    devmem::Owner<> mem;             // the buffers above
};
static int ensure_dev_callback_buffers(smcmi_handle *h) {
    if (h->dcbuf && h->dcbuf->n == h->n && h->dcbuf->d == h->d) return 0;
    delete h->dcbuf;
    h->dcbuf = nullptr;
    std::unique_ptr<DevCallbackBuffers> b(new DevCallbackBuffers());  // (installed only when complete; a failure below destroys it with what it made)
    b->mem.poison = sw().poison_alloc;
    b->n = h->n; b->d = h->d;
    const size_t n = (size_t)h->n, d = (size_t)h->d, nb = (n + TB - 1) / TB;
    if (dmalloc(b->mem, &b->d_pack, n * d) || dmalloc(b->mem, &b->d_out, n) || dmalloc(b->mem, &b->d_pos, n) || dmalloc(b->mem, &b->d_blk, nb + 1) || dmalloc(b->mem, &b->d_cnt, 2))
        return SMCMI_ERR_HIP;
    HIP_TRY(b->mem.alloc(&b->h_cnt, 2, devmem::Kind::Pinned));
    h->dcbuf = b.release();
    return 0;
}

// ---- kernels (wave64: __ballot is 64 bits wide; TB = 256 threads = 4 wavefronts, one row per thread, coalesced along the particle index)
// rows of this block that pass the gate, per wavefront in LDS; returns this row's rank among the block's passing rows
__device__ __forceinline__ long long dcb_block_rank(const bool pass, long long *wave_cnt /* [TB / 64], LDS */) {
    const unsigned long long bal = __ballot(pass);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wave; ++w) before += wave_cnt[w];
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}
static __global__ void __launch_bounds__(TB) k_dcb_count(const double *__restrict__ gate, long long n, long long *__restrict__ blk) {
    __shared__ long long wave_cnt[TB / 64];
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    const bool pass = i < n && gate[i] != SMCMI_NEG_INF;
    const unsigned long long bal = __ballot(pass);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long c = 0;
        for (int w = 0; w < TB / 64; ++w) c += wave_cnt[w];
        blk[blockIdx.x] = c;
    }
}
// one block: blk[0, nb) counts -> exclusive prefix sums in place, blk[nb] and cnt[0] = the total m
constexpr int DCB_ST = 1024;
static __global__ void __launch_bounds__(DCB_ST) k_dcb_scan(long long *__restrict__ blk, long long nb, long long *__restrict__ cnt) {
    __shared__ long long part[DCB_ST];
    const int t = threadIdx.x;
    const long long per = (nb + DCB_ST - 1) / DCB_ST, a = t * per < nb ? t * per : nb, b = a + per < nb ? a + per : nb;
    long long s = 0;
    for (long long k = a; k < b; ++k) s += blk[k];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < DCB_ST; off <<= 1) {             // inclusive scan of the 1024 segment sums
        const long long v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - s;
    for (long long k = a; k < b; ++k) { const long long c = blk[k]; blk[k] = run; run += c; }
    if (t == DCB_ST - 1) { blk[nb] = part[t]; cnt[0] = part[t]; }
}
// stable gather of the passing rows: pack[pos + m * j] = theta[i + n * j]; pos[i] = -1 for the others
static __global__ void __launch_bounds__(TB) k_dcb_pack(const double *__restrict__ theta, const double *__restrict__ gate, long long n, int d, long long m,
                                                        const long long *__restrict__ blk, double *__restrict__ pack, long long *__restrict__ pos) {
    __shared__ long long wave_cnt[TB / 64];
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    const bool pass = i < n && gate[i] != SMCMI_NEG_INF;
    const long long p = blk[blockIdx.x] + dcb_block_rank(pass, wave_cnt);
    if (i >= n) return;
    pos[i] = pass ? p : -1;
    if (pass && p < m)
        for (int j = 0; j < d; ++j) pack[p + m * j] = theta[i + n * j];
}
// lik[i] = -Inf where the bounds check failed, else the user's value with NaN -> -Inf; pos == nullptr: every row passed, out may be lik itself
static __global__ void __launch_bounds__(TB) k_dcb_scatter(const double *out, const long long *__restrict__ pos, long long n, long long m, double *lik) {
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long long p = pos ? pos[i] : i;
    double v = SMCMI_NEG_INF;
    if (p >= 0 && p < m) { v = out[p]; if (v != v) v = SMCMI_NEG_INF; }
    lik[i] = v;
}
// the initial draw's redraw loop: the rows still without a finite log-likelihood (attempt >= 0) whose fresh draw is inside the bounds are scored
static __global__ void __launch_bounds__(TB) k_dcb_init_gate(const int *__restrict__ attempt, const double *__restrict__ logprior, long long n, double *__restrict__ gate) {
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    gate[i] = (attempt[i] >= 0 && logprior[i] != SMCMI_NEG_INF) ? 0.0 : SMCMI_NEG_INF;
}
// ... rows that were done keep their value, a finite score ends a row's loop (attempt = -1), the others draw again; todo += rows that draw again
static __global__ void __launch_bounds__(TB) k_dcb_init_advance(int *__restrict__ attempt, double *__restrict__ lik, double *__restrict__ keep, long long n,
                                                                unsigned long long *__restrict__ todo) {
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    bool again = false;
    if (i < n) {
        if (attempt[i] < 0) lik[i] = keep[i];
        else {
            const double ll = lik[i];
            again = ll == SMCMI_NEG_INF || ll != ll;
            attempt[i] = again ? attempt[i] + 1 : -1;
        }
        keep[i] = lik[i];
    }
    const unsigned long long bal = __ballot(again);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(todo, (unsigned long long)__popcll(bal));
}

// Score the rows of the n x d column-major block `theta` (device, leading dimension n) whose `gate` is not -Inf with device callback `which`,
// results into `lik_out` (device, n; -Inf for the others): count -> [pack] -> the user's function -> scatter, all on the handle's stream.
// reuse_count: the gate is the one of the call before (the old-data callback of a tempered update) - its count and pack are still valid.
// A compiled program at `which` (program.hpp) is called from a kernel of the engine's own, so bounds gate, NaN -> -Inf and the evaluation count
// are that one launch: no count, no pack, no scatter, and nothing the host waits for (reuse_count is moot).
static int eval_device_callback(smcmi_handle *h, int which, const double *theta, const double *gate, double *lik_out, bool reuse_count = false) {
    DevCallbackBuffers *b = h->dcbuf;
    const long long n = h->n;
    const int d = h->d;
    const unsigned nb = (unsigned)((n + TB - 1) / TB);
    hipStream_t s = h->stream;
    double t0 = cb_now_ms();
    if (h->prog[which].kernel) {
        const program::Args a{theta, gate, n, n, d, h->d_prog_data[which], h->prog_rows[which], h->prog_cols[which],
                              h->d_prog_par[which], h->prog_npar[which], lik_out, h->d_prog_evals};
        const hipError_t e = (hipError_t)program::launch(h->prog[which], a, (void *)s);
        b->phase_ms[CBP_ENQUEUE] += cb_now_ms() - t0;
        if (e != hipSuccess) return set_err(SMCMI_ERR_HIP, std::string("launching the compiled likelihood: ") + hipGetErrorString(e));
        h->cb_calls += 1;
        return 0;
    }
    if (!reuse_count) {
        k_dcb_count<<<nb, TB, 0, s>>>(gate, n, b->d_blk);
        k_dcb_scan<<<1, DCB_ST, 0, s>>>(b->d_blk, (long long)nb, b->d_cnt);
        HIP_TRY(hipMemcpyAsync(b->h_cnt, b->d_cnt, sizeof(long long), hipMemcpyDeviceToHost, s));
        double t1 = cb_now_ms();
        b->phase_ms[CBP_ENQUEUE] += t1 - t0;
        HIP_TRY(hipStreamSynchronize(s));
        t0 = cb_now_ms();
        b->phase_ms[CBP_COUNT] += t0 - t1;
        b->m = b->h_cnt[0];
        if (b->m < 0 || b->m > n) return set_err(SMCMI_ERR_STATE, "device callback: the count of in-bounds proposals is out of range");
        if (b->m < n) {
            k_dcb_pack<<<nb, TB, 0, s>>>(theta, gate, n, d, b->m, b->d_blk, b->d_pack, b->d_pos);
            t1 = cb_now_ms();
            b->phase_ms[CBP_ENQUEUE] += t1 - t0;
            t0 = t1;
        }
    }
    const long long m = b->m;
    const bool packed = m < n;
    if (m > 0) {
        const int rc = h->dcb[which](packed ? b->d_pack : theta, (int64_t)m, (int64_t)(packed ? m : n), (int64_t)d, packed ? b->d_out : lik_out, (void *)s, h->dcb_ud[which]);
        const double t1 = cb_now_ms();
        b->phase_ms[CBP_CALL] += t1 - t0;
        t0 = t1;
        if (rc != 0) return set_err(SMCMI_ERR_CALLBACK, "the device likelihood callback returned " + std::to_string(rc));
        h->cb_calls += 1; h->cb_evals += m;
    }
    k_dcb_scatter<<<nb, TB, 0, s>>>(packed ? b->d_out : lik_out, packed ? b->d_pos : nullptr, n, m, lik_out);
    b->phase_ms[CBP_ENQUEUE] += cb_now_ms() - t0;
    return 0;
}

// The rows the program launches scored since the last collect, from the device's counter into cb_evals: once per run or stand-alone call
// (the stream is drained here; every caller is about to wait for it anyway).  prog_reset: the counter starts a run at 0.
static inline bool has_program(const smcmi_handle *h) { return h->prog[0].kernel != nullptr || h->prog[1].kernel != nullptr; }
static int prog_reset(smcmi_handle *h) {
    if (has_program(h)) HIP_TRY(hipMemsetAsync(h->d_prog_evals, 0, sizeof(unsigned long long) * program::EVAL_WORDS, h->stream));
    return 0;
}
static int prog_collect(smcmi_handle *h) {
    if (!has_program(h)) return 0;
    std::vector<unsigned long long> c((size_t)program::EVAL_WORDS, 0ull);
    HIP_TRY(hipMemcpyAsync(c.data(), h->d_prog_evals, sizeof(unsigned long long) * program::EVAL_WORDS, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_prog_evals, 0, sizeof(unsigned long long) * program::EVAL_WORDS, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < program::EVAL_SLOTS; ++k) h->cb_evals += (long long)c[(size_t)k * program::EVAL_STRIDE];
    return 0;
}

// A FUSED program (include/smcmi.h SMCMI_PROGRAM_FUSED) at the new vintage of a run that is not tempered: the whole n_mh_steps x n_blocks loop
// below is ONE launch of the program's own copy of the generic mutation kernel (fusedsrc.hpp smcmi_program_mutate = k_mutate<0, 1>'s body with
// the user's function where mutate_generic scores a proposal), with the bits of the split path.  Anything at the old vintage - a family, a
// callback, a program, a data prefix - keeps the split path.
static inline bool fused_mutation_serves(const smcmi_handle *h, bool tempered) {
    return h->prog[0].mutate != nullptr && !tempered && h->h_model.lik[1].family == SMCMI_LIK_NONE && h->h_model.lik_prefix == 0;
}
// The launch is launch_mutate's for the generic kernel (the staged proposal constants for n_para <= 13, h->nb_mut blocks of h->mut_T threads,
// lds::mutate's bytes), and it leaves the energy sums and maxima exactly when the last accept launch of the split path does.  Like k_mutate it
// is a no-op on a stage that did not go ahead.
// count: the launch is a stage's mutation (false: sent ahead of the verdict - run_callback counts it once the stage went ahead).
static int fused_mutation(smcmi_handle *h, bool count = true) {
    const double t0 = cb_now_ms();
    MutArgs ma{};
    ma.seed = h->cfg.seed; ma.gid0 = h->cfg.gid0;
    ma.stage_consts = h->d <= 13 ? 1 : 0;
    if (h->cb_energy) { ma.esum = h->d_esum_part; ma.emax = h->d_emax_part; }
    CloudPtrs cl = h->cl;
    const DevState *st = h->d_st;
    const ModelDev *md = h->d_model;
    double *acc = h->d_acc_part;
    int standalone = 0;
    const double *data = h->d_prog_data[0], *par = h->d_prog_par[0];
    long long rows = h->prog_rows[0], cols = h->prog_cols[0], n_par = h->prog_npar[0];
    unsigned long long *evals = h->d_prog_evals;
    void *args[] = {&cl, &st, &md, &ma, &acc, &standalone, &data, &rows, &cols, &par, &n_par, &evals};
    const hipError_t e = (hipError_t)program::launch_mutate(h->prog[0], (unsigned)h->nb_mut, (unsigned)h->mut_T, h->mut_lds, args, (void *)h->stream);
    h->dcbuf->phase_ms[CBP_ENQUEUE] += cb_now_ms() - t0;
    if (e != hipSuccess) return set_err(SMCMI_ERR_HIP, std::string("launching the fused likelihood program: ") + hipGetErrorString(e));
    if (count) h->cb_calls += 1;
    return 0;
}

// host_mutation for a device callback: per MH step x block propose (k_mutate<1>, plain n x d proposals + their log-priors) -> the user's
// function on the in-bounds ones (new data, and old data in a tempered update) -> accept (k_mutate<2>), in stream order on h->stream.
static int device_mutation(smcmi_handle *h, const smcmi_run_config *rc, bool tempered) {
    if (int e = ensure_dev_callback_buffers(h)) return e;
    if (fused_mutation_serves(h, tempered)) return fused_mutation(h);
    if (ensure_split_buffers(h)) return SMCMI_ERR_HIP;
    for (int step = 0; step < rc->n_mh_steps; ++step)
        for (int blk = 0; blk < rc->n_blocks; ++blk) {
            double t0 = cb_now_ms();
            MutArgs ma{};
            ma.seed = h->cfg.seed; ma.gid0 = h->cfg.gid0; ma.proposals = h->d_prop; ma.prop_logprior = h->d_prop_lp;
            ma.prop_qdiff = h->d_prop_q; ma.acc_count = h->d_acc_count; ma.block = blk; ma.step = step;
            ma.prop_chunk = 0;
            k_mutate<1><<<h->nb_mut, h->mut_T, h->mut_lds, h->stream>>>(h->cl, h->d_st, h->d_model, ma, h->d_acc_part, 0);
            h->dcbuf->phase_ms[CBP_ENQUEUE] += cb_now_ms() - t0;
            if (int e = eval_device_callback(h, 0, h->d_prop, h->d_prop_lp, h->d_lik_new)) return e;
            // (the old-data callback reuses the count and pack of the new-data callback - unless that one was a program, which made neither)
            if (tempered) { if (int e = eval_device_callback(h, 1, h->d_prop, h->d_prop_lp, h->d_lik_old, h->prog[0].kernel == nullptr)) return e; }
            t0 = cb_now_ms();
            ma.lik_new = h->d_lik_new; ma.lik_old_new = tempered ? h->d_lik_old : nullptr;
            ma.last = (step == rc->n_mh_steps - 1 && blk == rc->n_blocks - 1) ? 1 : 0;
            if (h->cb_energy && ma.last) { ma.esum = h->d_esum_part; ma.emax = h->d_emax_part; }
            k_mutate<2><<<h->nb_mut, h->mut_T, h->mut_lds, h->stream>>>(h->cl, h->d_st, h->d_model, ma, h->d_acc_part, 0);
            h->dcbuf->phase_ms[CBP_ENQUEUE] += cb_now_ms() - t0;
        }
    return 0;
}

// callback_fill_loglh for a device callback: the cloud's parameter columns, its logprior column as the gate, the requested column as output
static int device_fill_loglh(smcmi_handle *h, int which, int column) {
    if (int e = ensure_dev_callback_buffers(h)) return e;
    const long long n = h->n;
    double *c0 = h->cl.buf[0];
    if (int e = eval_device_callback(h, which, c0, c0 + (long long)(h->d + 1) * n, c0 + (long long)column * n)) return e;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return prog_collect(h);
}

// callback_init_from_prior for a device callback: the same draws (k_draw_prior, same attempt numbering), the same redraw loop, with the
// attempt counters, the gate and the kept scores on the device; per round the host reads the in-bounds count and the rows left to redraw
static int device_init_from_prior(smcmi_handle *h) {
    if (h->d > 64) return set_err(SMCMI_ERR_UNSUPPORTED, "device prior draws serve n_para <= 64");
    if (ensure_split_buffers(h)) return SMCMI_ERR_HIP;
    if (int e = ensure_dev_callback_buffers(h)) return e;
    DevCallbackBuffers *b = h->dcbuf;
    const long long n = h->n;
    const int d = h->d;
    const unsigned nb = (unsigned)((n + TB - 1) / TB);
    int *attempt = h->d_acc_count;
    double *gate = h->d_prop_q, *lik = h->d_lik_new, *keep = h->d_lik_old;          // (the split's buffers are idle outside a mutation)
    unsigned long long *todo_d = reinterpret_cast<unsigned long long *>(b->d_cnt + 1);
    HIP_TRY(hipMemsetAsync(attempt, 0, sizeof(int) * n, h->stream));
    long long todo = n;
    for (int round = 0; todo > 0; ++round) {
        if (round > 100000) return set_err(SMCMI_ERR_STATE, "initial draw: no finite-likelihood draw found");
        HIP_TRY(hipMemsetAsync(todo_d, 0, sizeof(unsigned long long), h->stream));
        k_draw_prior<<<nb, TB, 0, h->stream>>>(h->cl, h->d_model, h->cfg.seed, h->cfg.gid0, attempt);
        k_dcb_init_gate<<<nb, TB, 0, h->stream>>>(attempt, h->cl.buf[0] + (long long)(d + 1) * n, n, gate);
        if (int e = eval_device_callback(h, 0, h->cl.buf[0], gate, lik)) return e;
        k_dcb_init_advance<<<nb, TB, 0, h->stream>>>(attempt, lik, keep, n, todo_d);
        HIP_TRY(hipMemcpyAsync(b->h_cnt + 1, todo_d, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        todo = b->h_cnt[1];
    }
    HIP_TRY(hipMemcpyAsync(h->cl.buf[0] + (long long)d * n, lik, sizeof(double) * n, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return prog_collect(h);
}
