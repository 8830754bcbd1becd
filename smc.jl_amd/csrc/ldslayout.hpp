// ldslayout.hpp - the dynamic shared memory (LDS) of every stage kernel, described ONCE: its members in order, each with an element
// size, a count and an alignment.  The kernels take their pointers from these descriptions and the launch sites their byte counts
// (Layout::bytes): no kernel carves sm[] by hand, no launch site adds up a size of its own.  Plain C++17, no HIP: host and device
// code (constexpr functions) and tests/lds_check.cpp read the same text.  Static __shared__ arrays stay with their kernels.
#pragma once
#include <stddef.h>

#include <initializer_list>

#include "devstate.hpp"

namespace smcmi {

// ---- the constants the layouts are made of
constexpr int LIK_LDS_CAP = 768;          // doubles of likelihood data + regressors staged in LDS
constexpr int KALMAN4_SLOT_BYTES = 576;   // a particle's transposition slot of the four-lane Kalman filter (model.hpp kalman_lgss_quad)
constexpr int V2_MAXV = 8;                // virtual shards
constexpr int RMUT = 34;                  // mutation row: ES = 32 sums (energy power sums | Σ accept), [32] = energy maximum, [33] unused
constexpr int GRP = 64;                   // rows per canonical reduction group
constexpr int T3 = 512;                   // threads = particles of a segment block
constexpr int MT = 256;                   // particles per LDS tile of k_moments
constexpr int pad2(int m) { return (m + 1) & ~1; }   // row widths are even: rows are totalled with 16-byte loads (pad column = 0)

// what the proposal of the generic mutation kernel reads per block and per parameter, staged in LDS once per launch (in DevState / ModelDev
// they are global loads inside rolled loops: a dependent ~0.3-1 µs round trip per iteration with one wavefront per SIMD)
struct MutStage {
    double L[13 * 13], mu_b[13], sd_draw[13], sd_dens[13], logdet[13], lo[13], hi[13], prior_a[13], prior_b[13], prior_k[13];
    int block_ptr[14], blocks_all[13], l_off[13], fixed[13], prior_family[13];
};

namespace lds {

struct Member {
    size_t off, elem, count, align;       // bytes from sm[0]; element size; elements; alignment asked for
    int over;                             // -1, or the member this one deliberately shares its bytes with
    constexpr size_t end() const { return off + elem * count; }
};
template <int N>
struct Layout {
    Member m[N] = {};
    size_t at = 0;                        // end of the members placed so far
    size_t bytes = 0;                     // what a launch asks for: the members and the named slack behind them
    // the next member: `count` elements of `elem` bytes at the next multiple of `align` (0: of its element size)
    constexpr void put(int id, size_t count, size_t elem, size_t align = 0) {
        if (align == 0) align = elem;
        at = (at + align - 1) / align * align;
        m[id] = Member{at, elem, count, align, -1};
        at += elem * count;
    }
    // ... one that lives in the bytes of member `on` (and may reach past it): a declared overlay
    constexpr void overlay(int id, int on, size_t count, size_t elem, size_t align) {
        m[id] = Member{m[on].off, elem, count, align, on};
        if (m[id].end() > at) at = m[id].end();
    }
    constexpr void close(size_t slack = 0) { bytes = at + slack; }
    constexpr size_t operator[](int id) const { return m[id].off; }
};
constexpr size_t D8 = sizeof(double), I4 = sizeof(int);

// ---- the mutation body's arrays (k_mutate_reg, and the front of Mut2Lds: what a kernel that loads a finished proposal needs - k2b_mutate),
// then the scratch of engine 2's prologue (k2_prologue: totals, covariance, factorisation)
enum Mut2Id {
    M_Ls,                                 // [D*D] row-major with stride D, identity-padded
    M_mu, M_sdd, M_rb = M_sdd, M_sdn,     // [D] each: kept in place, no kernel reads them - but the segment kernel's MH step, which keeps
                                          // the Normal priors' reciprocal sds in the second (M_rb: ModelDev::prior_rb)
    M_red,                                // [red_n] the block reduction's wave sums (4 waves: k_mutate_reg; up to 8: engine 2)
    M_lo, M_hi, M_a, M_b, M_k,            // [D] each: bounds and prior constants
    M_lpar,                               // [2 * LIK_PAR_MAX]
    M_ldat,                               // [lik_cap] staged likelihood data (the generic body of n_para > 10 reads its data where it is: 0)
    M_Lraw,                               // [D*D] packed block factors as the prepare step wrote them
    M_logdet, M_mub, M_sddr, M_sdnr,      // [D] each, block order
    M_ball,                               // [D]: ints from here on; this one kept in place, no kernel reads it
    M_fix, M_fam, M_bptr /* [D + 1] */, M_loff, M_ballr /* [D + 1] */,
    M_BODY_N,
    M_svt = M_BODY_N,                     // [V2_MAXV][pad2(NPF)]: read with 16-byte loads
    M_stot,                               // [pad2(NPF) + 4]
    M_covl, M_sigf, M_Aw, M_Lw,           // [D*D] each
    M_mean, M_muf,                        // [D] each
    M_bfree, M_fi, M_fij,                 // [D] ints each
    M_N
};
struct Mut2Layout : Layout<M_N> {
    size_t body_bytes = 0;                // the launch of a kernel that uses the body alone
};
constexpr Mut2Layout mut2(int D, int red_n = 8, int lik_cap = LIK_LDS_CAP, bool prologue = true) {
    const size_t d = (size_t)D, npf = (size_t)(D + 1) * (D + 2) / 2 + 2, row = (size_t)pad2((int)npf);
    Mut2Layout l;
    l.put(M_Ls, d * d, D8, 16);
    for (int id : {M_mu, M_sdd, M_sdn}) l.put(id, d, D8);
    l.put(M_red, (size_t)red_n, D8);
    for (int id : {M_lo, M_hi, M_a, M_b, M_k}) l.put(id, d, D8);
    l.put(M_lpar, 2 * LIK_PAR_MAX, D8);
    l.put(M_ldat, (size_t)lik_cap, D8);
    l.put(M_Lraw, d * d, D8);
    for (int id : {M_logdet, M_mub, M_sddr, M_sdnr}) l.put(id, d, D8);
    l.put(M_ball, d, I4);
    l.put(M_fix, d, I4, 8);               // (an odd D leaves one int unused in front of it)
    l.put(M_fam, d, I4);
    l.put(M_bptr, d + 1, I4);
    l.put(M_loff, d, I4);
    l.put(M_ballr, d + 1, I4);
    // slack: the ints were budgeted as 6 D + 8 where the arrays take 6 D + 2 + (D & 1); 32 bytes paid for rounding s_vt at run time
    l.body_bytes = l.at + (6 - (D & 1)) * I4 + 32;
    if (!prologue) { l.close(l.body_bytes - l.at); return l; }
    l.put(M_svt, V2_MAXV * row, D8, 16);
    l.put(M_stot, row + 4, D8);
    for (int id : {M_covl, M_sigf, M_Aw, M_Lw}) l.put(id, d * d, D8);
    for (int id : {M_mean, M_muf}) l.put(id, d, D8);
    for (int id : {M_bfree, M_fi, M_fij}) l.put(id, d, I4);
    // slack: the scratch was budgeted from the end of the body's slack (it starts inside it), its V2_MAXV + 1 rows as NPF + 1 wide
    // where they are pad2(NPF), and 4 ints and 32 bytes on top
    l.close((l.body_bytes - l[M_svt]) + (V2_MAXV + 1) * (npf + 1 - row) * D8 + 4 * I4 + 32);
    return l;
}

// ---- the per-particle vectors of the generic mutation body (kernels.hpp mutate_generic), [d][T] each with the particle's column tid:
// one thread per particle (T = the block), or FOUR lanes per particle - then per wavefront, T = 16: θ, θ', then {draw, solve scratch}
// overlaid with the Kalman filter's 16 transposition slots (dead while the filter runs: the accepted proposal is copied from θ')
enum ColsId { C_th /* current θ */, C_tn /* proposed θ */, C_y /* z / draw */, C_v /* triangular-solve scratch */, C_slots, C_N };
constexpr Layout<C_N> mut_cols(int d, int T, int LS) {
    Layout<C_N> l;
    for (int id : {C_th, C_tn, C_y, C_v}) l.put(id, (size_t)d * T, D8);
    if (LS == 4) {
        l.overlay(C_slots, C_y, 16 * KALMAN4_SLOT_BYTES, 1, 16);
        l.at = (l.at + 15) / 16 * 16;     // (a wavefront's area is a multiple of 16 bytes)
    }
    l.close();
    return l;
}
constexpr int LS4_D = 13;                 // the lgss_kalman family: the four-lane kernels are sized for it whatever the model's n_para
constexpr int mutate_wave_bytes_ls4(int d) { return (int)mut_cols(d, 16, 4).bytes; }
// bytes of the vectors of a 256-thread block's particles (LS = 1: T of them; LS = 4: four wavefronts of 16)
constexpr size_t mut_cols_block_bytes(int d, int T, int LS) { return LS == 4 ? (size_t)4 * mutate_wave_bytes_ls4(LS4_D) : mut_cols(d, T, 1).bytes; }

// k_mutate: the vectors | red | the staged proposal constants (`staged`: the four-lane kernel always, otherwise n_para <= 13)
enum MutateId { G_cols, G_red /* [blockDim.x / 64] */, G_stage, G_N };
constexpr Layout<G_N> mutate(int d, int T, int LS, bool staged) {
    Layout<G_N> l;
    l.put(G_cols, mut_cols_block_bytes(d, T, LS), 1, 16);
    l.put(G_red, staged ? 8 : (size_t)T / 64, D8);             // (the stage sits 8 doubles behind red)
    if (staged) l.put(G_stage, 1, sizeof(MutStage), 8);
    else l.m[G_stage] = Member{l.at, sizeof(MutStage), 0, 8, -1};
    // slack: one thread per particle counted red's T / 64 doubles on top of the 8 in front of the stage
    l.close(staged && LS == 1 ? (size_t)T / 64 * D8 : 0);
    return l;
}

// k2w_mutate: Mut2Lds without staged likelihood data | the vectors
enum K2wId { W_mut2, W_cols, W_N };
constexpr Layout<W_N> k2w(int D, int LS) {
    Layout<W_N> l;
    l.put(W_mut2, mut2(D, 8, 0).bytes, 1, 16);
    l.put(W_cols, mut_cols_block_bytes(D, 256, LS), 1, 16);
    l.close(64);                          // slack: k_mutate's 8 doubles of red, which this kernel keeps in Mut2Lds
    return l;
}

// k_prepare_mutation: the n_free-sized arrays are packed for the model's n_free, the launch is sized for n_free = d
enum PrepId { P_tot /* [npairs] rounded up to 64 */, P_covl /* [d*d] */, P_sigf, P_A /* scaled block covariance */, P_Ls /* factor of the current block */, P_N };
constexpr Layout<P_N> prep(int d, int nf) {
    const size_t np = (size_t)(d + 1) * (d + 2) / 2;
    Layout<P_N> l;
    l.put(P_tot, (np + 63) / 64 * 64, D8, 16);
    l.put(P_covl, (size_t)d * d, D8);
    for (int id : {P_sigf, P_A, P_Ls}) l.put(id, (size_t)nf * nf, D8);
    l.close(3 * (size_t)(d * d - nf * nf) * D8 + 8 * D8);       // slack: 8 doubles
    return l;
}

// k_moments: a tile of MT particles, rows padded by one (pair threads reading different rows hit different banks)
enum MomId { O_xs /* da rows: row 0 = 1, row a+1 = θ_a - shift_a */, O_wv /* weights of the tile */, O_pa, O_pb /* the pair index decoded: a <= b */, O_N };
constexpr Layout<O_N> moments(int d) {
    const size_t np = (size_t)(d + 1) * (d + 2) / 2;
    Layout<O_N> l;
    l.put(O_xs, (size_t)(d + 1) * (MT + 1), D8, 16);
    l.put(O_wv, MT + 1, D8);
    l.put(O_pa, np, 1);
    l.put(O_pb, np, 1);
    l.close(16);                          // slack: 16 bytes
    return l;
}

// k3_segment, a worker: Mut2Lds | the parked draws of the next stage, slot-major (MH uniform, mixture uniform, D normals)[T3] | `cols`
// columns [T3]: the particle in transit through an in-place selection (D + 5, stage3.hpp k3_sel_cols), or the second chunk of a
// two-chunk worker (D + 6: θ_1..θ_D | loglh | logprior | old_loglh | accept | W | W̃).  A gatherer uses none of it: it stages its
// virtual shard's rows (at most 2 GRP of them, pad2(NPF) or RMUT columns) from sm[0] on.
enum Seg3Id { S_mut2, S_park, S_cols, S_gather, S_N };
constexpr int seg3_ch2_cols(int D) { return D + 6; }
struct Seg3Layout : Layout<S_N> {
    size_t gather_bytes = 0;              // what a launch with gatherers that stage rows must have at least
};
constexpr Seg3Layout seg3(int D, int cols) {
    const size_t row = (size_t)pad2((D + 1) * (D + 2) / 2 + 2);
    Seg3Layout l;
    l.put(S_mut2, mut2(D).bytes, 1, 16);
    l.put(S_park, (size_t)(D + 2) * T3, D8, 16);
    l.put(S_cols, (size_t)cols * T3, D8);
    l.close();
    l.gather_bytes = 2 * GRP * (row > (size_t)RMUT ? row : (size_t)RMUT) * D8;
    l.m[S_gather] = Member{0, D8, l.gather_bytes / D8, 16, S_mut2};
    return l;
}

// kens_run (enskernel.hpp), one workgroup = one whole run of `n` particles: the mutation body's arrays | every block's expanded factor |
// two particle-length arrays - the particles' energies (loglh - old_loglh), and their weights, which a selection turns into the cumulative
// weights it searches - | the scratch of the block reductions, the moments and the proposal
enum EnsId {
    X_body,                               // mut2(D, 4, LIK_LDS_CAP, false): what MutBodyLds::place_body<4, LIK_LDS_CAP> carves
    X_Ls,                                 // [D][D*D] the blocks' factors as expand_alpha1_factor leaves them (at most D blocks)
    X_en, X_wv,                           // [n] each
    X_red,                                // [4 * 64] block_reduce_many's wave rows
    X_tot,                                // [64] the totals a reduction leaves for every thread
    X_covl, X_sigf, X_A,                  // [D*D] each: covariance, its free symmetrised part, a block's scaled matrix
    X_mean, X_muf,                        // [D] each
    X_bfree, X_fi, X_fij,                 // [D] ints each
    X_N
};
constexpr Layout<X_N> ens(int D, long long n) {
    const size_t d = (size_t)D;
    Layout<X_N> l;
    l.put(X_body, mut2(D, 4, LIK_LDS_CAP, false).bytes, 1, 16);
    l.put(X_Ls, d * d * d, D8, 16);
    for (int id : {X_en, X_wv}) l.put(id, (size_t)n, D8);
    l.put(X_red, 4 * 64, D8);
    l.put(X_tot, 64, D8);
    for (int id : {X_covl, X_sigf, X_A}) l.put(id, d * d, D8);
    for (int id : {X_mean, X_muf}) l.put(id, d, D8);
    for (int id : {X_bfree, X_fi, X_fij}) l.put(id, d, I4);
    l.close();
    return l;
}

}  // namespace lds

// columns of LDS a segment kernel gets for the particle in transit (0: the particle is parked in device memory instead, Sel3Args::transit).
// The mixture variant carries T3 x D doubles of static z columns and the dense mixture block (k3_mix_static_bytes): with them and the
// D + 5 columns a block outgrows a CU's 160 KB beyond n_para 7.  K3_STATIC_REST: a bound on the rest of the kernel's static arrays,
// which tests/test_abi_cpu.py holds against the compiler's report.
constexpr size_t CU_LDS_BYTES = 160 * 1024, K3_STATIC_REST = 24 * 1024;
constexpr size_t k3_mix_static_bytes(int D) { return ((size_t)T3 * D + 3 * D * D + 3 * D + 3) * sizeof(double); }     // (T3 D z columns; MixDense<D>::DOUBLES + D D)
constexpr int k3_sel_cols(int D, bool alpha1) {
    return (alpha1 || K3_STATIC_REST + k3_mix_static_bytes(D) + lds::seg3(D, D + 5).bytes <= CU_LDS_BYTES) ? D + 5 : 0;
}
// a segment kernel's dynamic LDS with the columns its instantiation keeps behind the parking area (CH = 2: the second chunk), and the most
// a launch of it asks for - what the kernel is opted in to, in whole KB (launch2.hpp launch_k3_seg)
constexpr lds::Seg3Layout k3_layout(int D, bool alpha1, int CH) { return lds::seg3(D, CH == 2 ? lds::seg3_ch2_cols(D) : k3_sel_cols(D, alpha1)); }
constexpr size_t k3_max_lds_bytes(int D, bool alpha1, int CH) {
    const lds::Seg3Layout l = k3_layout(D, alpha1, CH);
    return ((CH == 2 || l.bytes > l.gather_bytes ? l.bytes : l.gather_bytes) + 1023) / 1024 * 1024;    // (a two-chunk launch asks for its layout alone)
}

}  // namespace smcmi
