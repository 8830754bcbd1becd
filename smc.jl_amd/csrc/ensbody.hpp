// ensbody.hpp - an ensemble of small SMC runs in ONE launch (include/smcmi.h smcmi_run_ensemble): kens_run<n_para>, one workgroup per
// member.  A workgroup runs the whole loop of src/smc_main.jl:377-508 on its member's cloud until ϕ = 1 - ϕ selection (the schedule, or
// the adaptive root by bracketing passes), correction and ESS, the resample decision, selection through a cumulative-weight scan and
// search, c, weighted mean and covariance, random blocks, the blocks' Cholesky factors, n_mh_steps x n_blocks MH proposals per particle,
// the acceptance rate, the records and history columns, the log-MDD - and leaves the member's DevState as a solo run leaves it.
// The hard rule: NO workgroup reads anything another workgroup of the launch writes.  There is no wait of one workgroup on another, no
// residency requirement, no time-out: a grid larger than the chip queues.
// What carries the Philox contract and the arithmetic of a proposal is the register mutation body of kernels.hpp (mh_draw, mh_step,
// expand_alpha1_factor, stage_lik, chol_rows_in_regs, MutBodyLds); the block reductions are block_reduce_many / block_max (DPP + LDS).
// α = 1 only (the driver refuses mixture proposals).  Compiled per n_para in translation units of their own (ens.hip, behind enskernel.hpp
// and its launcher).
// This header is the kernel's DEVICE part and depends on the device headers alone (kernels.hpp and what it includes, ensshape.hpp): the
// run-time compiler reads it too, for a likelihood given as HIP source and compiled for ensembles (include/smcmi.h
// smcmi_program_compile_ensemble, enssrc.hpp).  That translation unit defines SMCMI_PROGRAM_ENTRY, the user's function, and
// SMCMI_PROGRAM_ENS before it includes this file: the kernel's text below then is a device function its own kernel smcmi_program_ensemble
// calls, which scores a proposal with the user's function (model.hpp loglik_s, family SMCMI_LIK_PROGRAM) on the member's own data and
// parameters (EnsProg) and counts its calls.  Without the defines - every translation unit of the library - the macros expand to nothing
// or to the kernel's own head: the library compiles from the same tokens with or without those blocks.
#pragma once
#include "kernels.hpp"
#include "ensshape.hpp"

namespace smcmi {

// DevState in front of `sol` as start_state (runsetup.hpp) leaves it: a member's start travels in its table entry; what a run writes of
// DevState - up to the n_para x n_para entries of cov, like engines 2 / 3 - travels back in one row of words per member
constexpr size_t ENS_HEAD_BYTES = __builtin_offsetof(DevState, sol);
static_assert(ENS_HEAD_BYTES % 8 == 0 && sizeof(DevState) % 8 == 0 && __builtin_offsetof(DevState, cov) % 8 == 0, "DevState is copied as 8-byte words");
struct EnsHead { unsigned long long w[ENS_HEAD_BYTES / 8]; };
constexpr int ens_state_words(int d) { return (int)((__builtin_offsetof(DevState, cov) + (size_t)d * d * sizeof(double)) / 8); }
constexpr int ENS_OUT_WORDS = ens_state_words(ENS_MAX_D);

struct EnsMember {               // one row of the device-memory table: where a member's handle keeps its things
    double *cloud, *other;       // the current cloud buffer; the other one (a selection gathers into it)
    DevState *st;
    const ModelDev *md;
    Records rec;
    double *hist_w, *hist_W;     // null: no history kept
    unsigned long long seed;
    EnsHead head;
};
struct EnsArgs {
    const EnsMember *members;
    const double *sched;         // the proposed schedule of the call's run configuration (n_phi entries)
    unsigned long long *out;     // [members][ENS_OUT_WORDS]
    long long n;                 // particles of every member
};
// A member that carries a program (runens.hpp: every member of the call the same code object): one row of a table parallel to the members',
// the device copies of the data and parameters its registration was given, and the word its wavefronts add their evaluation counts to
struct EnsProg {
    const double *data;
    long long rows, cols;
    const double *par;
    long long n_par;
    unsigned long long *evals;
};
static_assert(sizeof(EnsProg) == 48, "six 8-byte words, to the library's compiler and to the run-time compiler");
#ifdef SMCMI_PROGRAM_ENS
#define SMCMI_ENS_PROG_PARAM , const EnsProg *progs
#define SMCMI_ENS_HEAD __device__ __forceinline__ void ens_run_body
#else
#define SMCMI_ENS_PROG_PARAM
#define SMCMI_ENS_HEAD __global__ void __launch_bounds__(ENS_T) kens_run
#endif

// totals of M accumulators per thread for EVERY thread: tot[0 .. M)
template <int M>
__device__ inline void ens_totals(double (&a)[M], double *red, double *tot) {
    const double v = block_reduce_many<M>(a, red);
    if ((int)threadIdx.x < M) tot[threadIdx.x] = v;
    __syncthreads();
}
__device__ inline double ens_max(double v, double *red) {
    const double m = block_max(v, red, ENS_T / 64);
    __syncthreads();                         // (the next reduction writes `red` without a barrier in front)
    return m;
}
constexpr int ens_pow2(int m) { return m <= 1 ? 1 : 2 * ens_pow2((m + 1) / 2); }
#ifdef SMCMI_PROGRAM_ENS
// The run-time compiler is an older LLVM than the one that builds the library: it leaves an array of more than 16 accumulators that goes
// through block_reduce_many in scratch memory (528 bytes per lane at n_para = 10).  Sixteen at a time it keeps them in registers.  An
// accumulator's total is the same xor butterfly over the lanes (32, 16, .. 1) and the same sum over the wavefronts whatever M is: the bits of
// ens_totals<M>.
template <int M>
__device__ __forceinline__ void ens_totals_wide(double (&a)[M], double *red, double *tot) {
    if constexpr (M <= 16) ens_totals<M>(a, red, tot);
    else {
#pragma unroll
        for (int c = 0; c < M / 16; ++c) {
            double part[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) part[k] = a[c * 16 + k];
            ens_totals<16>(part, red, tot + c * 16);
        }
    }
}
#define SMCMI_ENS_TOTALS ens_totals_wide
#else
#define SMCMI_ENS_TOTALS ens_totals
#endif

template <int D>
SMCMI_ENS_HEAD(EnsArgs a SMCMI_ENS_PROG_PARAM) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ unsigned long long s_head[ENS_HEAD_BYTES / 8];
    __shared__ int s_fail;
    constexpr int T = ENS_T, HW = (int)(ENS_HEAD_BYTES / 8), SW = ens_state_words(D);
    constexpr int NPAIR = D * (D + 1) / 2, M1 = ens_pow2(D + 1), M2 = ens_pow2(NPAIR);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_inf();
    const EnsMember *mp = a.members + blockIdx.x;
    double *const cloud = mp->cloud, *const other = mp->other;
    DevState *const st = mp->st;
    const ModelDev *const md = mp->md;
    const Records rec = mp->rec;
    double *const hist_w = mp->hist_w, *const hist_W = mp->hist_W;
    const unsigned long long seed = mp->seed;
    const long long n = a.n;
    const EnsShape shape = ens_shape(n, D);
    const auto O = lds::ens(D, n);
    MutBodyLds<D> B;
    B.template place_body<4, LIK_LDS_CAP>(sm);            // (lds::X_body sits at sm[0])
    double *const Ls = lds_at<double>(sm, O, lds::X_Ls), *const en = lds_at<double>(sm, O, lds::X_en), *const wv = lds_at<double>(sm, O, lds::X_wv);
    double *const red = lds_at<double>(sm, O, lds::X_red), *const tot = lds_at<double>(sm, O, lds::X_tot);
    double *const covl = lds_at<double>(sm, O, lds::X_covl), *const sig_f = lds_at<double>(sm, O, lds::X_sigf), *const A = lds_at<double>(sm, O, lds::X_A);
    double *const mean = lds_at<double>(sm, O, lds::X_mean), *const mu_f = lds_at<double>(sm, O, lds::X_muf);
    int *const bfree = lds_at<int>(sm, O, lds::X_bfree), *const fi = lds_at<int>(sm, O, lds::X_fi), *const fi_j = lds_at<int>(sm, O, lds::X_fij);

    // ---- the member's start: DevState = the head and zeros behind it, the model and the likelihood data into LDS (once per run)
    unsigned long long *const stw = reinterpret_cast<unsigned long long *>(st);
    for (int k = tid; k < HW; k += T) s_head[k] = mp->head.w[k];
    for (int k = tid; k < (int)(sizeof(DevState) / 8); k += T) stw[k] = k < HW ? mp->head.w[k] : 0ull;
    for (int k = tid; k < D; k += T) {
        B.m_lo[k] = md->lo[k]; B.m_hi[k] = md->hi[k]; B.m_a[k] = md->prior_a[k]; B.m_b[k] = md->prior_b[k]; B.m_k[k] = md->prior_k[k];
        B.m_fix[k] = md->fixed[k]; B.m_fam[k] = md->prior_family[k];
    }
    for (int k = tid; k < 2 * LIK_PAR_MAX; k += T) B.l_par[k] = md->lik[k / LIK_PAR_MAX].par[k % LIK_PAR_MAX];
    const LikDev ld0 = md->lik[0], ld1 = md->lik[1];
    const int has_other = md->has_other_priors, nf = md->n_free;
    for (int k = tid; k < nf; k += T) fi[k] = md->free_inds[k];
    const ModelView mv{D, B.m_fix, B.m_fam, B.m_lo, B.m_hi, B.m_a, B.m_b, B.m_k};
    LikView lv[2];
    stage_lik(ld0, ld1, B.l_par, B.l_dat, T, lv);
#ifdef SMCMI_PROGRAM_ENS
    // the member's program in place of its device family: the user's function reads the member's own copies of data and par, of any length
    const EnsProg pg = progs[blockIdx.x];
    lv[0] = LikView{SMCMI_LIK_PROGRAM, pg.par, 0.0, pg.data, pg.rows, pg.cols, nullptr, 0, 0, pg.n_par, 0ull};      // (scored: calls of the function by this thread)
#endif
    __syncthreads();
    DevState *const hd = reinterpret_cast<DevState *>(s_head);          // (only what stands in front of DevState::sol is touched)
    const RunParams rp = hd->rp;
    const double N = (double)rp.n_parts;
    const int nb = rp.n_blocks, n_steps = rp.n_mh_steps, n_phi = rp.n_phi;
    const bool hist = rp.store_history && hist_w != nullptr;
    for (int k = tid; k < rp.max_stages; k += T) rec.resampled[k] = 0;
    if (tid == 0) { rec.phi[0] = 0.0; rec.ess[0] = hd->ess_prev; rec.c[0] = hd->c; rec.accept[0] = hd->accept; }
    for (int q = 0; q < shape.per_thread; ++q) {
        const long long p = ens_particle(shape, n, tid, q);
        if (p < 0) continue;
        const double w0 = cloud[(long long)(D + 4) * n + p];
        en[p] = cloud[(long long)D * n + p] - cloud[(long long)(D + 2) * n + p];
        wv[p] = w0;
        if (hist) { hist_w[p] = 0.0; hist_W[p] = w0; }
    }
    __syncthreads();

    // ---- the loop scalars: every thread holds the same values (they come from block totals all threads read)
    int i = hd->stage, j = hd->j, rl = hd->resampled_last, rs = 0, resamples = hd->resamples, err = 0;
    double phi_n = hd->phi_n, phi_prop = hd->phi_prop, phi_prev = hd->phi_prev, c = hd->c, accept = hd->accept, ess_prev = hd->ess_prev;
    double ess = hd->ess, s1 = hd->sumw, s2 = hd->sumw2, logz = hd->logz;
    long long passes = hd->solver_passes;

    while (phi_n < 1.0) {
        if (i + 1 > rp.max_stages) { err = SMCMI_ERR_CAPACITY; break; }
        i += 1;
        const double phi_n1 = phi_n;
        // the energy shift of the stage's incremental weights: the largest finite energy of a particle that still has weight (any common
        // shift leaves W, the ESS and - with its factor put back - the log-MDD what they are; this one bounds every weight by 1)
        double em = -inf;
        for (int q = 0; q < shape.per_thread; ++q) {
            const long long p = ens_particle(shape, n, tid, q);
            if (p >= 0 && wv[p] > 0.0 && fabs(en[p]) < inf) em = fmax(em, en[p]);
        }
        em = ens_max(em, red);
        const double esh = fabs(em) < 1e300 ? em : 0.0;

        // ---- ϕ_n (smc_main.jl:378-396): the proposed schedule, or solve_adaptive_ϕ (helpers.jl:9-56)
        if (rp.use_fixed_schedule) phi_n = i <= n_phi ? a.sched[i - 1] : 1.0;
        else {
            const double ess_now = rl ? N : ess_prev, ess_bar = rp.tempering_target * ess_now;      // helpers.jl:14-20
            double cand[8], g[8];
            // ESS(ϕ) - ESS_bar at the eight candidates in one pass over the energies
            auto pass8 = [&]() {
                double acc[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] = 0.0;
                for (int q = 0; q < shape.per_thread; ++q) {
                    const long long p = ens_particle(shape, n, tid, q);
                    if (p < 0) continue;
                    const double e = en[p] - esh, w = wv[p];
#pragma unroll
                    for (int k = 0; k < 8; ++k) { const double v = weight_times(w, exp((cand[k] - phi_n1) * e)); acc[k] += v; acc[8 + k] += v * v; }
                }
                ens_totals<16>(acc, red, tot);
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = tot[k] * tot[k] / tot[8 + k] - ess_bar;
                passes += 1;
            };
            // the walk `while g(ϕ_prop) >= 0 && j <= n_Φ: ϕ_prop = schedule[j]; j += 1` (helpers.jl:29-32), eight schedule points per pass
            double lo = phi_n1, glo = ess_now - ess_bar, g_prop = 0.0;
            for (;;) {
                // (constant indices throughout: an array indexed by a run-time value lives in scratch memory)
                const int left = n_phi - j + 1, K = 1 + (left < 0 ? 0 : (left > 7 ? 7 : left));
                const int j0 = j;
                cand[0] = phi_prop;
#pragma unroll
                for (int k = 1; k < 8; ++k) cand[k] = k < K ? a.sched[j0 - 2 + k] : cand[k - 1];
                pass8();
                int k = 0;
                g_prop = g[0];
#pragma unroll
                for (int kk = 0; kk < 7; ++kk)
                    if (k == kk && kk < K - 1 && g[kk] >= 0.0) {
                        if (cand[kk] > lo) { lo = cand[kk]; glo = g[kk]; }
                        phi_prop = cand[kk + 1]; j += 1; k = kk + 1;
                        g_prop = g[kk + 1];
                    }
                if (!(g_prop >= 0.0 && j <= n_phi && k == K - 1 && K > 1)) break;
            }
            if (phi_prop != 1.0 || g_prop < 0.0) {
                // Roots.fzero(g, [ϕ_n1, ϕ_prop]) (helpers.jl:49) as a bracketing search, eight candidates per pass - the secant estimate with
                // rings around it and the bracket's quarter points -, certified to phi_rtol like the solver of the other engines
                // (kernels.hpp solver_decide_wave): the bracket's width against rtol ϕ, or short enough for linear interpolation between its
                // evaluated ends to be exact to that; rtol = 0: to adjacent floats
                double hi = phi_prop, ghi = g_prop;
                if (!(ghi < 0.0) || !(glo >= 0.0)) { err = SMCMI_ERR_BRACKET; i -= 1; break; }      // (g(ϕ_prop) is not a number: no bracket)
                const double rtol = rp.phi_rtol;
                for (int it = 0; it < 128; ++it) {
                    const double h = hi - lo;
                    const bool fin = glo < 1e300 && ghi > -1e300;
                    if (!(h > rtol * hi) || (fin && 64.0 * h * h <= rtol * hi * (hi - phi_n1))) break;
                    const double xs = lo + h * ((fin && glo > ghi) ? glo / (glo - ghi) : 0.5);
                    cand[0] = xs - h * 0x1p-4; cand[1] = xs - h * 0x1p-12; cand[2] = xs; cand[3] = xs + h * 0x1p-12; cand[4] = xs + h * 0x1p-4;
                    cand[5] = lo + h * 0.25; cand[6] = lo + h * 0.5; cand[7] = lo + h * 0.75;
                    const double mid = lo + h * 0.5;
                    bool any = false;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (!(cand[k] > lo && cand[k] < hi)) cand[k] = mid;
                        any = any || (cand[k] > lo && cand[k] < hi);
                    }
                    if (!any) break;                                  // no representable point inside: adjacent floats
                    pass8();
                    // the new bracket: the smallest candidate with g < 0 (or the old end), the largest one below it with g >= 0
                    double nhi = hi, nghi = ghi, nlo = lo, nglo = glo;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (cand[k] > lo && cand[k] < nhi && g[k] < 0.0) { nhi = cand[k]; nghi = g[k]; }
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (cand[k] > nlo && cand[k] < nhi && g[k] >= 0.0) { nlo = cand[k]; nglo = g[k]; }
                    if (nhi == hi && nlo == lo) { err = SMCMI_ERR_BRACKET; break; }      // (no candidate's ESS is a number)
                    hi = nhi; ghi = nghi; lo = nlo; glo = nglo;
                }
                if (err) { i -= 1; break; }
                double pn = (fabs(glo) <= fabs(ghi)) ? lo : hi;
                if (glo < 1e300 && ghi > -1e300) {                    // interpolate inside the certified bracket (glo == 0: lo)
                    const double xs = lo + (hi - lo) * (glo / (glo - ghi));
                    if (xs >= lo && xs <= hi) pn = xs;
                }
                phi_n = pn;
            } else phi_n = 1.0;                                        // helpers.jl:51-53
        }

        // ---- correction (smc_main.jl:401-420), ESS (:427), log-MDD increment
        const double dphi = phi_n - phi_n1;
        {
            double acc[2] = {0.0, 0.0};
            for (int q = 0; q < shape.per_thread; ++q) {
                const long long p = ens_particle(shape, n, tid, q);
                if (p < 0) continue;
                const double e = en[p], v = weight_times(wv[p], exp(dphi * (e - esh)));      // (a row of weight 0 adds 0 whatever its energy: kernels.hpp)
                wv[p] = v;
                acc[0] += v; acc[1] += v * v;
                if (hist) hist_w[(long long)(i - 1) * n + p] = exp(dphi * e);
            }
            ens_totals<2>(acc, red, tot);
        }
        phi_prev = phi_n1;
        s1 = tot[0]; s2 = tot[1];
        ess = s1 * s1 / s2;
        if (tid == 0) { rec.phi[i - 1] = phi_n; rec.ess[i - 1] = ess; }
        if (isnan(ess)) { err = SMCMI_ERR_NAN_ESS; break; }              // smc_main.jl:431
        logz += log(s1 / N) + dphi * esh;
        rs = ess < rp.threshold ? 1 : 0;                                   // :435
        __syncthreads();
        // normalize_weights! (particle.jl:362-366): W·N then /ΣW̃, two roundings like the reference
        for (int q = 0; q < shape.per_thread; ++q) {
            const long long p = ens_particle(shape, n, tid, q);
            if (p >= 0) wv[p] = (wv[p] * N) / s1;
        }
        __syncthreads();

        // ---- selection (smc_main.jl:435-446, resample.jl:23-72): cumsum(w / Σw) of w = W / N by a block scan over contiguous stretches, then
        // every slot searches its threshold and copies its ancestor's row into the other buffer (the mutation reads it there)
        if (rs) {
            double acc[1] = {0.0};
            long long beg, end;
            ens_chunk(shape, n, tid, beg, end);
            for (long long p = beg; p < end; ++p) acc[0] += wv[p] / N;
            ens_totals<1>(acc, red, tot);
            const double ssum = tot[0];
            double local = 0.0;
            for (long long p = beg; p < end; ++p) local += (wv[p] / N) / ssum;
            double incl = local;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const double up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            if (lane == 63) red[wave] = incl;
            __syncthreads();
            double run = incl - local;
            for (int w = 0; w < wave; ++w) run += red[w];
            // (a row of weight 0 keeps its cum value with the sign bit set: the selection rule below needs to know it, and wv is all there is)
            for (long long p = beg; p < end; ++p) { const double w0 = wv[p]; run += (w0 / N) / ssum; wv[p] = w0 > 0.0 ? run : -run; }
            __syncthreads();
            double u_sys = 0.0, ub_ = 0.0;
            if (rp.resampling_method != SMCMI_RESAMPLE_MULTINOMIAL) uniform_pair(seed, 0ull, (unsigned)i, rng_tag(P_RES, 0, 0), u_sys, ub_);
            for (int q = 0; q < shape.per_thread; ++q) {
                const long long p = ens_particle(shape, n, tid, q);
                if (p < 0) continue;
                double thr;
                if (rp.resampling_method == SMCMI_RESAMPLE_MULTINOMIAL) uniform_pair(seed, (unsigned long long)p, (unsigned)i, rng_tag(P_RES, 0, 0), thr, ub_);
                else thr = ((double)p + u_sys) / N;                          // (i - 1 + offset) / n_parts
                long long lo = 0, hi = n;                                     // first index with cum > thr
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (fabs(wv[mid]) > thr) hi = mid; else lo = mid + 1;
                }
                long long anc = lo < n ? lo : n - 1;                         // the selection rule (kernels.hpp select_rule): a fall-through or a
                while (anc > 0 && __builtin_signbit(wv[anc])) --anc;                   // row of weight 0 takes the nearest row before it with positive weight
#pragma unroll
                for (int k = 0; k < D + 3; ++k) other[(long long)k * n + p] = cloud[(long long)k * n + anc];
            }
            __syncthreads();
            for (int q = 0; q < shape.per_thread; ++q) {                     // reset_weights!
                const long long p = ens_particle(shape, n, tid, q);
                if (p >= 0) wv[p] = 1.0;
            }
            __syncthreads();
        }
        const double *const src = rs ? other : cloud;
        c = c * (0.95 + 0.10 * exp(16.0 * (accept - rp.target)) / (1.0 + exp(16.0 * (accept - rp.target))));      // :453-455
        if (tid == 0) { rec.c[i - 1] = c; rec.resampled[i - 1] = rs; }

        // ---- weighted mean and covariance (particle.jl:481-483, 526-529), two passes: the sums of the second are centred on the mean
        double sw;
        {
            double acc[M1];
#pragma unroll
            for (int k = 0; k < M1; ++k) acc[k] = 0.0;
            for (int q = 0; q < shape.per_thread; ++q) {
                const long long p = ens_particle(shape, n, tid, q);
                if (p < 0) continue;
                const double w = wv[p];
                acc[0] += w;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[1 + k] += w * src[(long long)k * n + p];
            }
            ens_totals<M1>(acc, red, tot);
            sw = tot[0];
            if (tid < D) mean[tid] = tot[1 + tid] / sw;
            __syncthreads();
        }
        {
            double acc[M2], mu[D];
#pragma unroll
            for (int k = 0; k < M2; ++k) acc[k] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) mu[k] = mean[k];
            for (int q = 0; q < shape.per_thread; ++q) {
                const long long p = ens_particle(shape, n, tid, q);
                if (p < 0) continue;
                const double w = wv[p];
                double xc[D];
#pragma unroll
                for (int k = 0; k < D; ++k) xc[k] = src[(long long)k * n + p] - mu[k];
                int pq = 0;
#pragma unroll
                for (int r = 0; r < D; ++r) {
                    const double wx = w * xc[r];
#pragma unroll
                    for (int s = r; s < D; ++s) { acc[pq] += wx * xc[s]; ++pq; }
                }
            }
            SMCMI_ENS_TOTALS<M2>(acc, red, tot);
            for (int e = tid; e < D * D; e += T) {
                int r = e / D, s = e % D;
                if (r > s) { const int tmp = r; r = s; s = tmp; }
                const double v = tot[r * D - r * (r - 1) / 2 + (s - r)] / sw;
                covl[e] = v;
                st->cov[e] = v;
            }
            if (tid < D) { st->mean[tid] = mean[tid]; st->shift[tid] = mean[tid]; }
        }

        // ---- random blocks (helpers.jl:215-260, Fisher-Yates on Philox) and per block c²Σ_b = L Lᵀ (mutation.jl:81), once per stage: the
        // arithmetic of k_prepare_mutation, results in LDS where the mutation body reads them
        if (tid == 0) s_fail = 0;
        if (tid >= 64 && tid < 128) {
            const int i0 = tid - 64;                 // lane i draws the Fisher-Yates partner of position i (independent Philox calls)
            if (i0 < nf) {
                bfree[i0] = i0;
                int jx = 0;
                if (i0 >= 1) {
                    double ua, ub;
                    uniform_pair(seed, 0ull, (unsigned)i, rng_tag(P_BLK, (unsigned)i0, 0), ua, ub);
                    jx = (int)(ua * (double)(i0 + 1));
                    if (jx > i0) jx = i0;
                }
                fi_j[i0] = jx;
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        if (tid == 64) {
            for (int k = nf - 1; k >= 1; --k) {
                const int jx = fi_j[k];
                const int tmp = bfree[k]; bfree[k] = bfree[jx]; bfree[jx] = tmp;
            }
            const int sub = (nf + nb - 1) / nb;
            for (int b = 0; b < nb; ++b) B.bptr_s[b] = b * sub;
            B.bptr_s[nb] = nf;
        }
        __syncthreads();
        // R_fr = (R[f,f] + R[f,f]')/2, θ_bar_fr (smc_main.jl:462-465)
        for (int e = tid; e < nf * nf; e += T) {
            const int r = fi[e / nf], s = fi[e % nf];
            sig_f[e] = (covl[r * D + s] + covl[s * D + r]) / 2.0;
        }
        for (int k = tid; k < nf; k += T) mu_f[k] = mean[fi[k]];
        __syncthreads();
        for (int k = tid; k < nf; k += T) {
            const int f = bfree[k];
            B.ball_raw[k] = fi[f];
            B.mub_raw[k] = mu_f[f];
            B.sdd_raw[k] = sqrt(c * c * sig_f[f * nf + f]);
            B.sdn_raw[k] = sqrt(sig_f[f * nf + f]);
        }
        int off = 0;
        for (int b = 0; b < nb; ++b) {
            const int p0 = B.bptr_s[b], db = B.bptr_s[b + 1] - p0;
            for (int e = tid; e < db * db; e += T) A[e] = c * c * sig_f[bfree[p0 + e / db] * nf + bfree[p0 + e % db]];
            for (int e = tid; e < db * db; e += T) B.Lraw[off + e] = 0.0;
            __syncthreads();
            // right-looking Cholesky inside ONE wavefront, lane r owns row r (chol_rows_in_regs: the subtraction order of the textbook loop)
            if (tid < 64) {
                double r[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) r[k] = (tid < db && k < db) ? A[tid * db + k] : 0.0;
                const bool ok = chol_rows_in_regs<12>(r, db, tid);
                if (!ok && tid == 0) s_fail = 1;
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (tid < db && k <= tid) B.Lraw[off + tid * db + k] = r[k];
            }
            __syncthreads();
            if (tid < 64) {                                // log of the diagonal in parallel, summed in index order
                const double lg = (tid < db) ? log(B.Lraw[off + tid * db + tid]) : 0.0;
                double ld = 0.0;
                for (int k = 0; k < db; ++k) ld += __shfl(lg, k, 64);
                if (tid == 0) { B.logdet_s[b] = 2.0 * ld; B.loff_s[b] = off; }
            }
            off += db * db;
            __syncthreads();
        }
        if (s_fail) { err = SMCMI_ERR_POSDEF; break; }                  // PosDefException aborts the run (mutation.jl:81)
        for (int b = 0; b < nb; ++b) {
            const int p0 = B.bptr_s[b], db = B.bptr_s[b + 1] - p0;
            expand_alpha1_factor<D>(Ls + b * D * D, B.Lraw + B.loff_s[b], B.ball_raw + p0, db, T, tid);
        }
        __syncthreads();

        // ---- mutation (mutation.jl:56-138): n_mh_steps x n_blocks proposals per particle, the register body of kernels.hpp
        double acc_sum = 0.0;
        for (int q = 0; q < shape.per_thread; ++q) {
            const long long p = ens_particle(shape, n, tid, q);
            if (p < 0) continue;
            double x[D];
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = src[(long long)k * n + p];
            double like = src[(long long)D * n + p], lprior = src[(long long)(D + 1) * n + p], like_prev = src[(long long)(D + 2) * n + p], acc_p = 0.0;
            for (int step = 0; step < n_steps; ++step)
                for (int b = 0; b < nb; ++b) {
                    const int db = B.bptr_s[b + 1] - B.bptr_s[b];
                    const unsigned t = (unsigned)(step * nb + b);
                    double step_prob, uc, z[D];
                    mh_draw<D>(seed, (unsigned long long)p, (unsigned)i, t, db, step_prob, uc, z);
                    mh_step<D, true, T>(Ls + b * D * D, B.logdet_s[b], db, nullptr, lv, mv, has_other, 0, rp.alpha, phi_n, (double *)nullptr, z, uc, step_prob, x,
                                        like, lprior, like_prev, acc_p);
                }
#pragma unroll
            for (int k = 0; k < D; ++k) cloud[(long long)k * n + p] = x[k];
            cloud[(long long)D * n + p] = like;
            cloud[(long long)(D + 1) * n + p] = lprior;
            cloud[(long long)(D + 2) * n + p] = like_prev;
            const double acc_val = acc_p / (double)nf;                   // quirk Q2: normalised by n_free only
            cloud[(long long)(D + 3) * n + p] = acc_val;
            const double w = wv[p];
            cloud[(long long)(D + 4) * n + p] = w;
            if (hist) hist_W[(long long)(i - 1) * n + p] = w;
            en[p] = like - like_prev;
            acc_sum += acc_val;
        }
        {
            double acc[1] = {acc_sum};
            ens_totals<1>(acc, red, tot);
        }
        accept = tot[0] / N;                                              // :484
        if (tid == 0) rec.accept[i - 1] = accept;
        ess_prev = ess; rl = rs; resamples += rs;
        __syncthreads();
    }

    // ---- what a solo run leaves in DevState, on the device and - one row of words per member - for the host's copy
    __syncthreads();
    if (tid == 0) {
        hd->stage = i; hd->j = j; hd->resampled_last = rl; hd->do_resample = rs; hd->done = 1; hd->err = err; hd->resamples = resamples;
        hd->phi_prev = phi_prev; hd->phi_n = phi_n; hd->phi_prop = phi_prop; hd->ess_prev = ess_prev; hd->ess = ess_prev; hd->sumw = s1; hd->sumw2 = s2;
        hd->logz = logz; hd->c = c; hd->accept = accept; hd->solver_passes = passes;
    }
    __syncthreads();
    for (int k = tid; k < HW; k += T) stw[k] = s_head[k];
    __syncthreads();
    unsigned long long *const out = a.out + (long long)blockIdx.x * ENS_OUT_WORDS;
    for (int k = tid; k < SW; k += T) out[k] = stw[k];
#ifdef SMCMI_PROGRAM_ENS
    // the rows this workgroup scored: every wavefront sums its lanes' tallies and ends with ONE 64-bit atomic add, by lane 0 when the sum is
    // not 0, to the member's own word
    unsigned long long calls = lv[0].scored;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) calls += __shfl_xor(calls, off, 64);
    if (lane == 0 && calls != 0ull) atomicAdd(pg.evals, calls);
#endif
}

}  // namespace smcmi
