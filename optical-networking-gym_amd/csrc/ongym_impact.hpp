// ongym_impact.hpp — what each candidate action would do to the running lightpaths (ongym_action_impact, include/ongym.h):
// per replica and per action of a caller's list, the running services that share a link with the action's route (the
// victims), their GSNR with the candidate added as one more interferer, and how many of them fall below their threshold.
//
// The GN model is additive in the interferers (core/osnr.pyx:64-93), so a victim's 1/GSNR after the candidate is provisioned
// is its current 1/GSNR plus ONE term: gn_eval's per-interferer term with the roles swapped (the pair-table row is the
// candidate's slot count, Phi the candidate's format, the link weights summed over the links both cross), scaled by the
// victim's nli_coef[n_i] P^2.  This is calculate_osnr(victim) inside measure_disruptions right after the provisioning
// (envs/qrmsa.pyx:937-953).
//
// Kernel: one wavefront per replica on the step kernels' set-up (Ctx, load_state).
//   0. the routes the action list names (lanes over actions) and the OR of their link masks
//   1. baseline: 1/GSNR of every running record that crosses one of those links into `bef` f64[C] in LDS - k_service_qot's
//      evaluation (gn_build_list with the record left out, gn_eval), or, with svc_in, 10^(-ASE/10) + 10^(-NLI/10) of a
//      service_qot result on the same state (lanes over records, no GN evaluation at all)
//      The two "below" decisions on that baseline are made once per record (two bits in the LDS copy of the release times,
//      which this kernel neither reads nor stores back).
//   2. per action (wave-uniform loop): decode and is_path_free as evaluate_action does, then lanes over records, two per
//      lane and iteration with every load issued first: overlap test on the link mask, one 16-byte pair-table gather (every
//      lane reads the candidate's row), the shared links' weights, after = before + term, the two "below" decisions on it in
//      the linear domain (below_lane), per-lane counts, the largest after / limit (the lowest margin) with its record and
//      the largest after / before (the largest drop); the wave reduces them with DPP and converts the two maxima with one
//      log10: no logarithm per victim.
// Nothing is stored back: state, statistics and counters are untouched.
//
// LDS: the state block | lim0 f64[8] | 1/lim0 f64[8] | minimum_osnr f64[8] | bef f64[C].  NSFNET-320, C = 448:
// 8 208 + 192 + 3 584 = 11 984 B, ten 1 280-byte granules, 12 replicas per CU (k_service_qot: 8 544 B, seven granules, 18).  The alternative, C/64 register
// pairs per lane, needs a compile-time capacity; `bef` in LDS keeps one instantiation per layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"
#include "ongym_qot.hpp"

namespace ongym {

constexpr int kActionImpact = ONGYM_N_ACTION_IMPACT;   // impact_out doubles per (replica, action)
constexpr int kMaxImpactActions = ONGYM_MAX_IMPACT_ACTIONS;

__host__ __device__ inline size_t impact_lds_bytes(const Params &P) {
    return (lds_bytes(P) + 192 + (size_t)P.capacity * 8 + 15) & ~(size_t)15;
}

// (route, format, slot) of a step action index for the current request, as evaluate_action decodes it.
// 0 decoded; 1 not a placement (negative, the reject action, beyond it); 2 no such format / route / slot count
__device__ __forceinline__ int impact_decode(const Ctx &c, int action, int src, int dst, int max_mod, int &path, int &slot, int &n,
                                             int &m) {
    const Params &P = c.P;
    const int M = P.n_mods_consider, S = P.n_slots;
    if (action < 0 || action >= P.k_paths * M * S) return 1;
    slot = action % S;
    const int t = action / S, r = t % M, route = t / M;
    m = max_mod > 1 ? max_mod - r : (M - 1) - r;                 // allowed_mods (envs/qrmsa.pyx:821-825)
    if (m < 0 || m >= P.n_mods) return 2;
    path = G(P.pair_paths)[(src * P.n_nodes + dst) * P.k_paths + route];
    n = c.nreq[m];
    if (path < 0 || n <= 0) return 2;
    return 0;
}

// per-lane accumulators of one action
struct ImpactAcc {
    int cnt = 0, bel = 0, new0 = 0, newm = 0, qi = 0x7FFFFFFF;
    double qmax = -1.0, dmax = 0.0;            // largest after / limit and after / before: both positive
};

// one victim of the candidate: record i with the links `m0`, `m1` it shares with the candidate's route, format mi, centre
// distance adi (half slots), its pair-table entry (ta, tb) when `tab`, its coefficient k = nli_coef[n_i] P^2, its baseline and
// the baseline's two "below" decisions `was`
template <bool UA>
__device__ __forceinline__ void impact_victim(const Ctx &c, ImpactAcc &acc, int i, uint64_t m0, uint64_t m1, int mi, int adi, bool tab,
                                              double ta, double tb, double k, double before, uint32_t was, double bk, double phic,
                                              double margin, const double *lim0, const double *rlim0, const double *thr0) {
    const Params &P = c.P;
    double term = 0.0;
    if (UA) {
        double Aa, corr;
        if (tab) {
            Aa = ta;
            corr = phic * tb;
        } else {
            const double adf = (0.5 * P.slot_bw) * (double)adi, ck = P.alpha0_cl * bk;
            Aa = asinh_diff(ck * (adf + 0.5 * bk), ck * (adf - 0.5 * bk));   // adf > bk/2: the spectrum is free
            corr = phic * (bk / adf);
        }
        double w1 = 0.0, w2 = 0.0;
        while (m0) { const int l = __ffsll((unsigned long long)m0) - 1; m0 &= m0 - 1; w1 += c.lw[2 * l]; w2 += c.lw[2 * l + 1]; }
        while (m1) { const int l = 64 + __ffsll((unsigned long long)m1) - 1; m1 &= m1 - 1; w1 += c.lw[2 * l]; w2 += c.lw[2 * l + 1]; }
        term = Aa * w1 - corr * w2;
    } else {
        const double adf = (0.5 * P.slot_bw) * (double)adi;
        const double hi = adf + 0.5 * bk, lo = adf - 0.5 * bk, corr = phic * (bk / adf);
        while (m0 | m1) {
            int l;
            if (m0) { l = __ffsll((unsigned long long)m0) - 1; m0 &= m0 - 1; }
            else { l = 64 + __ffsll((unsigned long long)m1) - 1; m1 &= m1 - 1; }
            const double ck = c.lcl[l] * bk;
            term += asinh_diff(ck * hi, ck * lo) * c.lw[2 * l] - corr * c.lw[2 * l + 1];
        }
    }
    const double after = before + k * term;
    const double thr = thr0[mi];
    const bool b0a = below_lane(after, lim0[mi], thr);              // measure_disruptions' test (qrmsa.pyx:947)
    const bool bma = below_lane(after, c.lim[mi], thr + margin);    // !qot_ok
    const bool b0b = (was & 1u) != 0, bmb = (was & 2u) != 0;        // the same two tests on `before`, made once per record
    acc.cnt++;
    acc.bel += b0a;
    acc.new0 += b0a && !b0b;
    acc.newm += bma && !bmb;
    const double q = after * rlim0[mi];
    if (q > acc.qmax) { acc.qmax = q; acc.qi = i; }                 // ascending i per lane: the lowest index on a tie
    acc.dmax = fmax(acc.dmax, after / before);
}

template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_action_impact(const Params *__restrict__ Pp, int A, const int32_t *__restrict__ actions,
                                                      const double *__restrict__ svc_in, double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    double *lim0 = reinterpret_cast<double *>(smem + lds_bytes(P));
    double *rlim0 = lim0 + 8, *thr0 = rlim0 + 8, *bef = thr0 + 8;
    const int C = P.capacity, K = P.k_paths, lane = c.lane;
    if (lane < P.n_mods) {
        lim0[lane] = pow(10.0, -P.mod_thr[lane] / 10.0);                    // the expression of load_state
        rlim0[lane] = pow(10.0, P.mod_thr[lane] / 10.0);
        thr0[lane] = P.mod_thr[lane];
    }
    load_state(c);                                                          // (its wave_sync orders the stores above)
    const int active = c.active;
    const DevEnv *e = c.e;
    const bool have = uniform_i32(e->have_request) != 0;
    const int src = uniform_i32(e->cur_src), dst = uniform_i32(e->cur_dst), cur_id = uniform_i32(e->cur_id);
    const int max_mod = uniform_i32(e->st.max_modulation_idx);
    const double margin = e->margin, lp2 = c.rp[1];
    const auto *acts = G(actions) + (size_t)c.replica * A;
    double *orow = out + (size_t)c.replica * A * kActionImpact;

    // ---- 0. links of the routes the list names (a route whose spectrum turns out not to be free still counts: a superset)
    uint64_t um0 = 0, um1 = 0;
    if (have) {
        uint32_t used_lo = 0, used_hi = 0;
        for (int a = lane; a < A; a += kWave) {
            const int action = acts[a];
            if (action >= 0 && action < K * P.n_mods_consider * P.n_slots) {
                const int route = min(action / (P.n_slots * P.n_mods_consider), 63);
                if (route < 32) used_lo |= 1u << route; else used_hi |= 1u << (route - 32);
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) { used_lo |= __shfl_xor(used_lo, s); used_hi |= __shfl_xor(used_hi, s); }
        const uint64_t used = uniform_i32((int)used_lo) | ((uint64_t)(uint32_t)uniform_i32((int)used_hi) << 32);
        for (int k = 0; k < K; k++) {
            if (!((used >> min(k, 63)) & 1ull)) continue;
            const int path = uniform_i32(G(P.pair_paths)[(src * P.n_nodes + dst) * K + k]);
            if (path >= 0) { um0 |= G(P.path_mask)[2 * path]; um1 |= G(P.path_mask)[2 * path + 1]; }
        }
    }

    // ---- 1. baseline: 1/GSNR of every record on those links
    if (svc_in) {
        const auto *sv = G(svc_in) + (size_t)c.replica * C * kServiceQot;
        for (int i = lane; i < active; i += kWave)
            bef[i] = pow(10.0, -sv[kServiceQot * i + 1] / 10.0) + pow(10.0, -sv[kServiceQot * i + 2] / 10.0);
    } else if (um0 | um1) {
        for (int iy = 0; iy < active; iy++) {
            const uint32_t ay = c.sa[iy], by = c.sb[iy];
            const int py = uniform_i32(rec_path<R32>(ay, by));
            uint64_t ym0, ym1;
            if (R32) { ym0 = (uint32_t)uniform_i32((int)ay); ym1 = 0; }
            else { ym0 = G(P.path_mask)[2 * py]; ym1 = G(P.path_mask)[2 * py + 1]; }
            if (!uniform_i32(((ym0 & um0) | (ym1 & um1)) != 0)) continue;
            const GnLin g = gn_running<UA, R32>(c, iy);
            if (lane == 0) bef[iy] = g.ase + g.nli;
        }
    }
    wave_sync();
    // the two "below" decisions of every baseline, once per record.  They take the place of the release times in LDS, which
    // this kernel never reads (the sign bit that marks a disrupted service included) and never stores back.
    uint32_t *was = reinterpret_cast<uint32_t *>(c.sr);
    for (int i = lane; i < active; i += kWave) {
        const int mi = rec_mod<R32>(c.sa[i], c.sb[i]);
        const double b = bef[i], thr = thr0[mi];
        was[i] = (below_lane(b, lim0[mi], thr) ? 1u : 0u) | (below_lane(b, c.lim[mi], thr + margin) ? 2u : 0u);
    }
    wave_sync();

    // ---- 2. every action of the list
    int last_path = -1;
    PathRef p;
    p.m0 = p.m1 = 0; p.hops = 0; p.mylink = 0;
    uint64_t ext = 0;
    for (int a = 0; a < A; a++) {
        const int action = uniform_i32(acts[a]);
        int path = -1, slot = 0, n = 0, m = 0;
        int status = have ? uniform_i32(impact_decode(c, action, src, dst, max_mod, path, slot, n, m)) : 1;
        if (status == 0) {
            path = uniform_i32(path); slot = uniform_i32(slot); n = uniform_i32(n); m = uniform_i32(m);
            if (path != last_path) { p = load_path(c, path); ext = path_free_ext(c, p); last_path = path; }
            int rr = 1;
            const uint64_t ok_starts = run_and(ext, rr, n + 1);             // is_path_free, envs/qrmsa.pyx:1248-1264
            const uint64_t w = readlane_u64(ok_starts, slot >> 6);
            if (!((w >> (slot & 63)) & 1ull)) status = 2;
        }
        double *o = orow + (size_t)a * kActionImpact;
        if (status) {
            if (lane < kActionImpact) o[lane] = lane == 0 ? (double)status : NAN;
            continue;
        }
        // the candidate as an interferer: its width, centre and format are wave-uniform
        const int c2 = 2 * slot + n;
        const double bk = P.slot_bw * n, phic = c.phi[m];
        const bool tab = UA && n <= P.tab_nmax;
        const auto *trow = G(reinterpret_cast<const double *>(P.pair_tab)) + (tab ? 2 * (size_t)(n - 1) * P.tab_stride : 0);
        ImpactAcc acc;
        // two chunks of 64 records per iteration, and every load of both records - the record, its mask, the pair-table
        // entry, the victim's coefficient, its baseline - issued before the first use: the gathers are the latency of this loop.
        // A record that is no victim (or lies beyond `active`: zeros) still reads in bounds: its centre distance is <= 2S.
        for (int base = 0; base < active; base += 2 * kWave) {
            const int i0 = base + lane, i1 = i0 + kWave;
            const bool v0 = i0 < active, v1 = i1 < active;
            const uint32_t ra0 = v0 ? c.sa[i0] : 0u, rb0 = v0 ? c.sb[i0] : 0u, ra1 = v1 ? c.sa[i1] : 0u, rb1 = v1 ? c.sb[i1] : 0u;
            uint64_t m00, m01, m10, m11;
            if (R32) { m00 = ra0 & (uint32_t)p.m0; m10 = ra1 & (uint32_t)p.m0; m01 = m11 = 0; }
            else {
                const int pk0 = ra0 & 0xFFFF, pk1 = ra1 & 0xFFFF;
                m00 = G(P.path_mask)[2 * pk0] & p.m0; m01 = G(P.path_mask)[2 * pk0 + 1] & p.m1;
                m10 = G(P.path_mask)[2 * pk1] & p.m0; m11 = G(P.path_mask)[2 * pk1 + 1] & p.m1;
            }
            const int ni0 = rec_n<R32>(ra0, rb0), ni1 = rec_n<R32>(ra1, rb1);
            const int adi0 = abs((2 * rec_slot<R32>(ra0, rb0) + ni0) - c2), adi1 = abs((2 * rec_slot<R32>(ra1, rb1) + ni1) - c2);
            double ta0 = 0.0, tb0 = 0.0, ta1 = 0.0, tb1 = 0.0;
            if (tab) { ta0 = trow[2 * adi0]; tb0 = trow[2 * adi0 + 1]; ta1 = trow[2 * adi1]; tb1 = trow[2 * adi1 + 1]; }
            const double k0 = G(P.nli_coef)[ni0] * lp2, k1 = G(P.nli_coef)[ni1] * lp2;
            const double bef0 = bef[v0 ? i0 : 0], bef1 = bef[v1 ? i1 : 0];
            const uint32_t was0 = was[v0 ? i0 : 0], was1 = was[v1 ? i1 : 0];
            bool on0 = v0 && (m00 | m01) != 0, on1 = v1 && (m10 | m11) != 0;
            if (P.track_ids) {                                              // the request's namesakes never see it (quirk Q12)
                if (on0 && c.sq[i0] == (uint32_t)cur_id) on0 = false;
                if (on1 && c.sq[i1] == (uint32_t)cur_id) on1 = false;
            }
            if (on0) impact_victim<UA>(c, acc, i0, m00, m01, rec_mod<R32>(ra0, rb0), adi0, tab, ta0, tb0, k0, bef0, was0, bk, phic, margin, lim0, rlim0, thr0);
            if (on1) impact_victim<UA>(c, acc, i1, m10, m11, rec_mod<R32>(ra1, rb1), adi1, tab, ta1, tb1, k1, bef1, was1, bk, phic, margin, lim0, rlim0, thr0);
        }
        int cnt = acc.cnt, bel = acc.bel, new0 = acc.new0, newm = acc.newm, qi = acc.qi;
        double qmax = acc.qmax, dmax = acc.dmax;
        cnt = wave_sum_i32(cnt);
        bel = wave_sum_i32(bel);
        new0 = wave_sum_i32(new0);
        newm = wave_sum_i32(newm);
        dmax = wave_max_f64(dmax);
        const double qtop = wave_max_f64(qmax);                              // largest after / limit: the lowest margin
        qi = -wave_max_i32(qmax == qtop ? -qi : -0x7FFFFFFF);                //   ... and the lowest record index that has it
        if (lane < kActionImpact) {
            const bool any = cnt > 0;
            const double db = 10.0 * log10(lane == 5 ? qtop : dmax);         // one logarithm for both columns
            const double v[kActionImpact] = {0.0, (double)cnt, (double)bel, (double)new0, (double)newm, any ? -db : NAN,
                                             any ? db : NAN, any ? (double)qi : -1.0};
            double r = v[0];
            for (int k = 1; k < kActionImpact; k++) r = lane == k ? v[k] : r;
            o[lane] = r;
        }
    }
}

}  // namespace ongym
