// ongym_admission.hpp — first-fit admission of every node pair and bit rate (ongym_admission_map, include/ongym.h): per replica
// and per candidate action of a caller's list, which requests (unordered node pair q, bit rate r) first fit would still admit
// on the replica's state once the candidate is provisioned, where, and why not.
//
// Kernel: one wavefront per (replica, action, group) on the step kernels' set-up (Ctx, load_state), grid (batch, A, G).  Every
// wavefront works on its own LDS copy of the replica and stores nothing back.
//   0. the slot count and the GN coefficients of every (rate, format) into two registers per lane (entry r * 8 + m in lane
//      (r * 8 + m) % 64), read back with v_readlane: no LDS beyond the state block
//   1. the action decoded as k_action_impact decodes it; a candidate whose slots are free is provisioned as the step provisions
//      (mark_links, the guard slot unless it ends at S) and appended to the records as the step appends an accept
//   2. the group's share of the node pairs, a contiguous range in pair order.  Per pair, route-major: load_path and
//      path_free_ext once per route, gn_build_list once per route and only if some start is evaluated, then per undecided rate
//      (a register bit mask) the formats from the highest down as policy_first_fit searches them: run_and extended format by
//      format and restarted when a slot count shrinks, the lowest valid start only, the exact ASE lower bound where first fit
//      uses it, gn_eval / qot_ok over everything running in the scenario.  A probe has no service id (skip_id = -1) and is
//      never provisioned: cells do not see each other.  Lane r keeps the cell (q, r): its code, 1/GSNR and threshold; one
//      log10 per pair converts all its margins.
//   3. the weighted sums run over the cells in pair order, rate by rate, in every lane alike (wave-uniform adds, no atomics).
//      G = 1: the wavefront writes the scenario's summary row.  G > 1: it writes its partial sums, and k_admission_reduce adds
//      them in group order.
// Every loop is bounded by K, M, R, Q, N or the loaded `active`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"
#include "ongym_impact.hpp"        // impact_decode

namespace ongym {

constexpr int kAdmissionMap = ONGYM_N_ADMISSION_MAP;   // summary_out doubles per (replica, action)
constexpr int kMaxAdmissionRates = ONGYM_MAX_ADMISSION_RATES;
constexpr int kMaxAdmissionActions = ONGYM_MAX_ADMISSION_ACTIONS;
constexpr int kAdmissionPart = 10;        // partial sums per (replica, action, group): status, admitted, blocked for spectrum,
                                          // blocked on QoT, sum w, sum w rate (blocked), sum w rate (all), lowest margin, detoured, -

struct AdmissionRates { float v[kMaxAdmissionRates]; };   // travels with the launch

// partial sums -> the eight columns of a summary row
__device__ __forceinline__ void admission_row(double *o, int status, double adm, double ns, double qt, double bp, double num,
                                              double den, double low, double det) {
    const bool ok = status < 2;
    o[0] = (double)status;
    o[1] = ok ? adm : NAN;
    o[2] = ok ? ns : NAN;
    o[3] = ok ? qt : NAN;
    o[4] = ok ? bp : NAN;
    o[5] = ok ? num / den : NAN;
    o[6] = ok && adm > 0.0 ? low : NAN;
    o[7] = ok ? det : NAN;
}

template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_admission_map(const Params *__restrict__ Pp, int A, const int32_t *__restrict__ actions, int R,
                                                      AdmissionRates rates, const double *__restrict__ weights, int NG,
                                                      double *__restrict__ summary, double *__restrict__ part,
                                                      int32_t *__restrict__ map_out, float *__restrict__ margin_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    const int C = P.capacity, K = P.k_paths, M = P.n_mods, S = P.n_slots, N = P.n_nodes, lane = c.lane;
    const int Q = N * (N - 1) / 2, grp = blockIdx.z;
    const int q0 = (int)((long long)Q * grp / NG), q1 = (int)((long long)Q * (grp + 1) / NG);
    const size_t scen = (size_t)c.replica * A + blockIdx.y;
    load_state(c);
    c.skip_id = -1;                                                         // a probe has no id: nobody is left out (quirk Q12)
    const DevEnv *e = c.e;
    const bool have = uniform_i32(e->have_request) != 0;
    const double margin = e->margin;

    // ---- 0. slots and coefficients of every (rate, format): entry t = r * 8 + m, lane t % 64, register t / 64
    double rate_l = 0.0;                                                    // lane r: rate r
#pragma unroll
    for (int r = 0; r < kMaxAdmissionRates; r++) rate_l = (lane == r && r < R) ? (double)rates.v[r] : rate_l;
    int n_t[2];
    double nlic_t[2], selfa_t[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int t = lane + 64 * h, r = t >> 3, m = t & 7;
        n_t[h] = 0; nlic_t[h] = 0.0; selfa_t[h] = 0.0;
        const double rate = __shfl(rate_l, r & (kMaxAdmissionRates - 1));   // rate of this lane's entry (lane r holds rate r)
        if (r < R && m < M) {
            const double v = ceil(rate / ((double)P.mod_se[m] * P.nslots_width));   // the step's expression (load_state)
            if (v >= 1.0 && v <= (double)S) {
                n_t[h] = (int)v;
                nlic_t[h] = G(P.nli_coef)[n_t[h]] * c.rp[1];
                selfa_t[h] = G(P.self_asinh)[n_t[h]];
            }
        }
    }

    // ---- 1. the candidate
    int status = 1;
    if (actions && have) {
        const int action = uniform_i32(G(actions)[scen]);
        const int src = uniform_i32(e->cur_src), dst = uniform_i32(e->cur_dst);
        int path = -1, slot = 0, n = 0, m = 0;
        status = uniform_i32(impact_decode(c, action, src, dst, uniform_i32(e->st.max_modulation_idx), path, slot, n, m));
        if (status == 0) {
            path = uniform_i32(path); slot = uniform_i32(slot); n = uniform_i32(n); m = uniform_i32(m);
            const PathRef p = load_path(c, path);
            int rr = 1;
            const uint64_t ok_starts = run_and(path_free_ext(c, p), rr, n + 1);   // is_path_free, envs/qrmsa.pyx:1248-1264
            const uint64_t w = readlane_u64(ok_starts, slot >> 6);
            if (!((w >> (slot & 63)) & 1ull)) status = 2;
            else if (c.active >= C) status = 3;
            else {                                                          // provisioned and appended as the step does
                int end = slot + n;
                if (end < S) end += 1;
                mark_links<false>(c, p.hops, p.mylink, slot, end, false);
                if (lane == 0) {
                    uint32_t ra, rb;
                    rec_pack<R32>(path, p.m0, slot, n, m, ra, rb);
                    c.sa[c.active] = ra; c.sb[c.active] = rb;
                    if (P.track_ids) c.sq[c.active] = (uint32_t)e->cur_id;
                }
                c.active++;
                wave_sync();
            }
        }
    }
    double *prow = part ? part + (scen * NG + grp) * kAdmissionPart : nullptr;
    const size_t cell0 = scen * (size_t)Q * R;
    if (status >= 2) {
        for (int i = q0 * R + lane; i < q1 * R; i += kWave) {
            if (map_out) map_out[cell0 + i] = -1;
            if (margin_out) margin_out[cell0 + i] = NAN;
        }
        if (lane == 0) {
            if (prow) prow[0] = (double)status;
            else admission_row(summary + scen * kAdmissionMap, status, 0, 0, 0, 0, 0, 0, 0, 0);
        }
        return;
    }

    // ---- 2. the group's pairs
    int s = 0, d;
    {
        int q = q0;
        while (s < N - 2 && q >= N - 1 - s) { q -= N - 1 - s; s++; }
        d = s + 1 + q;
    }
    const int reject = K * M * S;
    const uint32_t full = R >= 32 ? ~0u : ((1u << R) - 1u);
    const double wuni = 1.0 / ((double)Q * (double)R);
    int adm = 0, ns = 0, qt = 0, det = 0;
    double bp = 0.0, num = 0.0, den = 0.0, low_l = INFINITY;
    for (int q = q0; q < q1; q++) {
        uint32_t decided = 0, refused = 0;
        int code = reject;                                                  // lane r: cell (q, r)
        double acc_l = 1.0, thr_l = 0.0;
        const double w_l = lane < R ? (weights ? G(weights)[(size_t)q * R + lane] : wuni) : 0.0;   // in flight over the search
        for (int k = 0; k < K && decided != full; k++) {
            const int path = uniform_i32(G(P.pair_paths)[(s * N + d) * K + k]);
            if (path < 0) break;
            const PathRef p = load_path(c, path);
            const uint64_t ext = path_free_ext(c, p);
            uint64_t runs = ext;
            int rr = 1, L = -1;
            for (int r = 0; r < R; r++) {
                if ((decided >> r) & 1u) continue;
                for (int mm = M - 1; mm >= 0; mm--) {
                    const int t = r * 8 + mm;
                    const int nn = t < 64 ? __builtin_amdgcn_readlane(n_t[0], t) : __builtin_amdgcn_readlane(n_t[1], t - 64);
                    if (nn < 1) continue;                                   // unusable: n < 1 or n > S
                    if (nn + 1 < rr) { runs = ext; rr = 1; }
                    runs = run_and(runs, rr, nn + 1);
                    const int first = first_set(runs);
                    if (first < 0) continue;
                    GnCoef kf;
                    kf.nlic = t < 64 ? readlane_f64(nlic_t[0], t) : readlane_f64(nlic_t[1], t - 64);
                    kf.selfa = t < 64 ? readlane_f64(selfa_t[0], t) : readlane_f64(selfa_t[1], t - 64);
                    if (P.ase_shortcut) {                                   // exact lower bound, see policy_first_fit
                        const double bw = P.slot_bw * nn;
                        const double fc = P.f0 + (P.slot_bw * first) + (P.slot_bw * (nn / 2.0));
                        double lb = (bw * fc * p.ase) * c.rp[0];
                        if (UA) lb += kf.nlic * (p.w1 * kf.selfa);
                        if (uniform_i32(lb >= c.lim[mm] * (1.0 + kQotBand))) { refused |= 1u << r; continue; }
                    }
                    if (L < 0) L = gn_build_list<R32>(c, p.m0, p.m1);
                    const GnLin g = gn_eval<UA, R32>(c, p, L, first, nn, kf);
                    if (!qot_ok(c, g, mm, margin)) { refused |= 1u << r; continue; }
                    decided |= 1u << r;
                    if (lane == r) {
                        code = k * M * S + (M - 1 - mm) * S + first;
                        acc_l = uniform_f64(g.ase) + uniform_f64(g.nli);
                        thr_l = P.mod_thr[mm];
                    }
                    adm++;
                    det += k > 0;
                    break;
                }
            }
        }
        // the pair's R cells: lane r converts and stores cell r
        const bool mine = lane < R, in = mine && ((decided >> lane) & 1u);
        if (mine && !in && ((refused >> lane) & 1u)) code = reject + 1;
        const double mg = in ? -10.0 * log10(acc_l) - thr_l - margin : NAN;
        if (in) low_l = fmin(low_l, mg);
        if (mine) {
            if (map_out) map_out[cell0 + (size_t)q * R + lane] = code;
            if (margin_out) margin_out[cell0 + (size_t)q * R + lane] = (float)mg;
        }
        const int lost_q = __popc(refused & ~decided);
        qt += lost_q;
        ns += R - __popc(decided) - lost_q;
        const double wr_l = w_l * rate_l;
        for (int r = 0; r < R; r++) {                                       // fixed order: pair-major, then the rates
            const double w = readlane_f64(w_l, r), wr = readlane_f64(wr_l, r);
            den += wr;
            if (!((decided >> r) & 1u)) { bp += w; num += wr; }
        }
        if (++d == N) { s++; d = s + 1; }
    }
    const double low = -wave_max_f64(-low_l);
    if (lane == 0) {
        if (prow) {
            prow[0] = (double)status; prow[1] = adm; prow[2] = ns; prow[3] = qt; prow[4] = bp; prow[5] = num; prow[6] = den;
            prow[7] = low; prow[8] = det; prow[9] = 0.0;
        } else admission_row(summary + scen * kAdmissionMap, status, adm, ns, qt, bp, num, den, low, det);
    }
}

// G > 1: the groups' partial sums in group order, one thread per scenario
__global__ __launch_bounds__(256) void k_admission_reduce(size_t n_scen, int NG, const double *__restrict__ part,
                                                          double *__restrict__ summary) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_scen) return;
    const double *p = part + i * NG * kAdmissionPart;
    const int status = (int)p[0];
    double adm = 0.0, ns = 0.0, qt = 0.0, bp = 0.0, num = 0.0, den = 0.0, low = INFINITY, det = 0.0;
    if (status < 2)
        for (int g = 0; g < NG; g++, p += kAdmissionPart) {
            adm += p[1]; ns += p[2]; qt += p[3]; bp += p[4]; num += p[5]; den += p[6]; low = fmin(low, p[7]); det += p[8];
        }
    admission_row(summary + i * kAdmissionMap, status, adm, ns, qt, bp, num, den, low, det);
}

}  // namespace ongym
