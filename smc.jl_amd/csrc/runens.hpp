// runens.hpp - the host side of smcmi_run_ensemble (include/smcmi.h): many whole-cloud handles, one launch, one workgroup per member
// (enskernel.hpp).  The call enqueues a number of launches that does not depend on the stage count - one - and there is no per-stage host
// work: the members' start state travels in ONE copy of the member table (pointers into every handle's own buffers and the head of its
// fresh DevState), their stage-1 records and first history columns are written by the kernel, their closed loop states come back in ONE
// copy.  Argument checks, schedule, RunParams, the fresh DevState and the result fill are runsetup.hpp's.  Included by smcmi.hip behind
// run2.hpp.
// Members that carry a program compiled for ensembles (smcmi_program_compile_ensemble, enssrc.hpp) run the same way through the program's own
// copy of the kernel, smcmi_program_ensemble: one hipModuleLaunchKernel of member 0's function - every member carries the same code object -
// with a table parallel to the members' that holds each one's data, parameters and evaluation counter (EnsProg).  The counters sit in the
// call's buffer between what goes up (as zeros) and what comes back: still one upload and one download.
#pragma once
#include "enskernel.hpp"

static_assert(ENS_HEAD_BYTES == ST_HEAD_BYTES, "the member table carries DevState's head as a fresh run's prologue does");
static_assert(ens_state_words(ENS_MAX_D) == res2_state_words(ENS_MAX_D), "a member's row holds what a run of engines 2 / 3 hands back");

static inline bool h0_prog(const smcmi_handle *h) { return h->prog[0].ensemble != nullptr; }      // an ensemble program at SMCMI_WHICH_NEW

// the refusals of the call as a whole: nothing has run and no handle has changed when one of them returns
static int check_ensemble(smcmi_handle **hs, int32_t n, const smcmi_run_config *rc) {
    if (!hs || n < 1 || !rc) return set_err(SMCMI_ERR_ARG, "bad argument");
    for (int k = 0; k < n; ++k)
        if (!hs[k]) return set_err(SMCMI_ERR_ARG, "null handle in the ensemble");
    {
        std::vector<smcmi_handle *> sorted(hs, hs + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return set_err(SMCMI_ERR_ARG, "a handle is listed twice in the ensemble");
    }
    const smcmi_config &c0 = hs[0]->cfg;
    for (int k = 1; k < n; ++k) {
        const smcmi_config &c = hs[k]->cfg;
        if (c.device != c0.device || c.n_para != c0.n_para || c.n_parts != c0.n_parts || c.max_stages != c0.max_stages || c.store_history != c0.store_history)
            return set_err(SMCMI_ERR_ARG, "ensemble members must share device, n_para, n_parts, max_stages and store_history");
    }
    for (int k = 0; k < n; ++k) {
        const smcmi_handle *h = hs[k];
        if (h->cfg.n_local != h->cfg.n_parts || h->cfg.gid0 != 0) return set_err(SMCMI_ERR_UNSUPPORTED, "an ensemble member is a whole cloud, not a shard");
        if (closure_lik(h, 1) || (closure_lik(h, 0) && !h->prog[0].ensemble))
            return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble members evaluate device likelihood families or a program compiled for ensembles (smcmi_program_compile_ensemble) at SMCMI_WHICH_NEW: no host or device callbacks, no plain or fused programs");
        if (h->h_model.lik[1].family != SMCMI_LIK_NONE) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs take no old-data likelihood (tempered updates run through smcmi_run)");
    }
    // programs: every member or none, one code object, compiled for the members' n_para
    const bool prog = h0_prog(hs[0]);
    for (int k = 0; k < n; ++k) {
        if (h0_prog(hs[k]) != prog) return set_err(SMCMI_ERR_ARG, "ensemble members either all carry the same ensemble program or all evaluate device likelihood families");
        if (prog && hs[k]->prog[0].id != hs[0]->prog[0].id) return set_err(SMCMI_ERR_ARG, "ensemble members must carry the same ensemble program (one code object)");
        if (prog && hs[k]->prog[0].ens_para != c0.n_para) return set_err(SMCMI_ERR_ARG, "the ensemble program was compiled for another n_para than the members'");
    }
    if (rc->tempered_update_prior_weight != 0.0) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs take no tempered_update_prior_weight");
    if (rc->stop_after_stage > 0 || rc->continue_run) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs neither pause nor continue");
    if (c0.n_para > ENS_MAX_D) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs serve n_para <= 10");
    if (c0.n_parts > SMCMI_ENS_MAX_PARTS) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs serve n_parts <= SMCMI_ENS_MAX_PARTS");
    if (rc->alpha != 1.0) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs serve alpha = 1 (mixture proposals run through smcmi_run)");
    if (!ens_shape(c0.n_parts, c0.n_para).ok) return set_err(SMCMI_ERR_UNSUPPORTED, "ensemble runs: no launch shape for this cloud");
    for (int k = 0; k < n; ++k) {
        if (int e = need_model(hs[k], h0_prog(hs[k]) ? 2 : 1)) return e;      // (a program is a likelihood the kernels evaluate here)
        if (int e = check_run_config(hs[k], rc)) return e;
    }
    return 0;
}

static int launch_kens_d(int d, const EnsArgs &a, int n_members, hipStream_t stream) {
    switch (d) {
#define SMCMI_ENS_CASE(X, D) case D: return launch_kens<D>(a, n_members, stream);
        SMCMI_LAUNCH_ENS_D(SMCMI_ENS_CASE, )
#undef SMCMI_ENS_CASE
    default: return SMCMI_ERR_UNSUPPORTED;
    }
}

static int run_ensemble_impl(smcmi_handle **hs, int32_t n, const smcmi_run_config *rc, smcmi_result *res, int32_t *status) {
    if (!res) return set_err(SMCMI_ERR_ARG, "null result");
    if (int e = check_ensemble(hs, n, rc)) return e;
    const auto t0 = std::chrono::steady_clock::now();
    smcmi_handle *h0 = hs[0];
    const int d = h0->d;
    HIP_TRY(hipSetDevice(h0->cfg.device));
    hipStream_t stream = h0->stream;
    // what the caller left on the members' own streams (an initial draw, an upload from the device) goes in front of the launch
    devmem::Handles made;
    for (int k = 1; k < n; ++k) {
        if (hipStreamQuery(hs[k]->stream) == hipSuccess) continue;             // nothing pending there
        hipEvent_t ev = nullptr;
        HIP_TRY(made.event(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, hs[k]->stream));
        HIP_TRY(hipStreamWaitEvent(stream, ev, 0));
    }
    // the member table | the proposed schedule | the members' result rows: one device buffer of 8-byte words that lives for the call
    const std::vector<double> sched = make_schedule(rc);
    static_assert(sizeof(EnsMember) % 8 == 0, "the table is copied as 8-byte words");
    // (program members: | the members' EnsProg rows | their evaluation counters, zeros on the way up and the first words of the way back)
    const bool prog = h0_prog(h0);
    static_assert(sizeof(EnsProg) % 8 == 0, "the table is copied as 8-byte words");
    const size_t tbl_words = (size_t)n * sizeof(EnsMember) / 8, sched_words = sched.size(), out_words = (size_t)n * ENS_OUT_WORDS;
    const size_t prog_words = prog ? (size_t)n * sizeof(EnsProg) / 8 : 0, eval_words = prog ? (size_t)n : 0;
    std::vector<unsigned long long> up(tbl_words + sched_words + prog_words + eval_words, 0ull), back(eval_words + out_words);
    for (int k = 0; k < n; ++k) {
        smcmi_handle *h = hs[k];
        if (int e = start_state(h, rc, make_run_params(h, rc), false, false)) return e;
        EnsMember m{};
        const int cur = h->h_st.cur & 1;
        m.cloud = h->cl.buf[cur]; m.other = h->cl.buf[cur ^ 1];
        m.st = h->d_st; m.md = h->d_model; m.rec = h->rec;
        m.hist_w = h->cfg.store_history ? h->d_hist_w : nullptr; m.hist_W = h->cfg.store_history ? h->d_hist_W : nullptr;
        m.seed = h->cfg.seed;
        memcpy(&m.head, &h->h_st, ENS_HEAD_BYTES);                              // (start_state: everything behind these bytes is zero)
        memcpy(up.data() + (size_t)k * sizeof(EnsMember) / 8, &m, sizeof(EnsMember));
    }
    memcpy(up.data() + tbl_words, sched.data(), sizeof(double) * sched.size());
    devmem::Owner<> tmp;
    unsigned long long *dbuf = nullptr;
    HIP_TRY(tmp.alloc(&dbuf, up.size() + out_words));
    unsigned long long *const d_evals = dbuf + up.size() - eval_words;
    for (int k = 0; prog && k < n; ++k) {
        const smcmi_handle *h = hs[k];
        const EnsProg pg{h->d_prog_data[0], (long long)h->prog_rows[0], (long long)h->prog_cols[0], h->d_prog_par[0], (long long)h->prog_npar[0], d_evals + k};
        memcpy(up.data() + tbl_words + sched_words + (size_t)k * sizeof(EnsProg) / 8, &pg, sizeof(EnsProg));
    }
    HIP_TRY(hipMemcpyAsync(dbuf, up.data(), sizeof(unsigned long long) * up.size(), hipMemcpyHostToDevice, stream));
    EnsArgs a{};
    a.members = reinterpret_cast<const EnsMember *>(dbuf);
    a.sched = reinterpret_cast<const double *>(dbuf + tbl_words);
    a.out = dbuf + up.size();
    a.n = h0->n;
    if (prog) {
        const EnsProg *progs = reinterpret_cast<const EnsProg *>(dbuf + tbl_words + sched_words);
        const EnsShape sh = ens_shape(a.n, d);
        void *args[] = {&a, &progs};
        const hipError_t e = (hipError_t)program::launch_ensemble(h0->prog[0], (unsigned)n, (unsigned)sh.block, sh.lds_bytes, args, (void *)stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return set_err(SMCMI_ERR_HIP, std::string("launching the ensemble program: ") + hipGetErrorString(e)); }
    } else if (int e = launch_kens_d(d, a, n, stream)) return e == SMCMI_ERR_HIP ? set_err(e, "the ensemble launch failed") : set_err(e, "ensemble runs: no kernel for this n_para");
    HIP_TRY(hipMemcpyAsync(back.data(), d_evals, sizeof(unsigned long long) * back.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t1 = std::chrono::steady_clock::now();
    int first = 0;
    for (int k = 0; k < n; ++k) {
        smcmi_handle *h = hs[k];
        if (prog) { h->cb_calls = 1; h->cb_evals = (long long)back[(size_t)k]; }        // smcmi_callback_stats: one launch, the rows this member's workgroup scored
        memcpy(&h->h_st, back.data() + eval_words + (size_t)k * ENS_OUT_WORDS, sizeof(unsigned long long) * (size_t)ens_state_words(d));
        h->h_st.e_shift = 0.0;                  // (as pull_state: the shift belongs to a running stage chain)
        h->last_n_stages = h->h_st.stage;
        h->center_stale = false;
        smcmi_result &r = res[k];
        memset(&r, 0, sizeof(r));
        finish_result(&r, h->h_st, t0, t1);
        const int code = h->h_st.err;
        if (status) status[k] = code;
        if (code && !first) first = code;
    }
    return first ? err_from_state(first) : 0;
}
