// ongym_failure.hpp — single-link failures and first-fit restoration (ongym_failure_impact, include/ongym.h): per replica and
// per failed link of a caller's list, the running lightpaths that cross the link (the victims), how many of them find another
// place through the spectrum that is left over at acceptable QoT, and what that costs in hops and slots.  Below it, the same
// for a SET of failed links per scenario (ongym_failure_sets, k_failure_sets): dual cuts, node failures, shared-risk groups.
//
// Kernel: one wavefront per (replica, failed link) scenario, grid (batch, F), on the step kernels' set-up (Ctx, load_state).
// Every scenario works on its own LDS copy of the replica and stores nothing back.
//   1. split the records in place (lanes over records, one ballot per chunk of 64): a victim's words go to the saved list in
//      record order, a survivor moves down to the next free position, so the survivors keep their order
//   2. release every victim like a departure of the step: [slot, slot + n + 1) clamped at S on every link of its route
//   3. per victim in record order (wave-uniform loop), first fit's search (policy_first_fit) with the victim's capacity
//      n * se[m] as the request: the routes of its node pair that avoid the failed link, formats from the highest down, the
//      lowest valid start only, the exact ASE lower bound where first fit uses it, then gn_build_list / gn_eval / qot_ok over
//      everything that runs in the scenario at that moment.  The first placement that passes is provisioned (mark_links, the
//      guard slot unless it ends at S) and appended to the records as the step appends an accept, so later victims see its
//      spectrum and its interference.
// Every loop is bounded by `active`, K, M or the row words.
//
// LDS: the state block | vsb u32[C] | (vsq u32[C] with id tracking) | vidx u16[C].  The victims' first record words `vsa` take
// the place of the release times `sr`, which this kernel never reads and never stores back.  NSFNET-320, C = 448:
// 8 208 + 2 688 = 10 896 B, nine 1 280-byte granules, 14 scenarios per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

constexpr int kFailureImpact = ONGYM_N_FAILURE_IMPACT;   // link_out doubles per (replica, failed link)

__host__ __device__ inline size_t failure_lds_bytes(const Params &P) {
    return (lds_bytes(P) + (size_t)P.capacity * (P.track_ids ? 10 : 6) + 15) & ~(size_t)15;
}

// slots of capacity `cap` (slots x spectral efficiency of the original) under a format of spectral efficiency `se`
__host__ __device__ inline int failure_slots(int cap, int se) { return (cap + se - 1) / se; }

template <bool R32>
__device__ __forceinline__ bool rec_on_link(const Params &P, uint32_t a, int link) {
    if (R32) return ((a >> link) & 1u) != 0;
    return ((G(P.path_mask)[2 * (int)(a & 0xFFFF) + (link >> 6)] >> (link & 63)) & 1ull) != 0;
}

template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_failure_impact(const Params *__restrict__ Pp, int F, const int32_t *__restrict__ links,
                                                       const int32_t *__restrict__ path_pair, double *__restrict__ link_out,
                                                       int32_t *__restrict__ svc_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    const int C = P.capacity, K = P.k_paths, M = P.n_mods, S = P.n_slots, lane = c.lane, f = blockIdx.y;
    uint32_t *vsb = reinterpret_cast<uint32_t *>(smem + lds_bytes(P));
    uint32_t *vsq = P.track_ids ? vsb + C : nullptr;                        // without id tracking vidx lies there
    uint16_t *vidx = reinterpret_cast<uint16_t *>(vsb + (P.track_ids ? 2 : 1) * (size_t)C);
    const size_t col = (size_t)c.replica * F + f;
    double *o = link_out + col * kFailureImpact;
    int32_t *srow = svc_out ? svc_out + col * C : nullptr;
    const int link = uniform_i32(links ? G(links)[col] : f);
    if (srow) {
        for (int i = lane; i < C; i += kWave) srow[i] = -1;
        __threadfence();                                                    // the victims' entries are stored over these below
    }
    if (link < 0 || link >= P.n_links) {
        if (lane < kFailureImpact) o[lane] = lane == 0 ? 1.0 : NAN;
        return;
    }
    load_state(c);
    uint32_t *vsa = reinterpret_cast<uint32_t *>(c.sr);                     // (load_state's wave_sync orders its stores to `sr`)
    const double margin = c.e->margin;

    // ---- 1. victims to the saved list, survivors moved down, both in record order
    const int active0 = c.active;
    int nv = 0, ns = 0;
    for (int base = 0; base < active0; base += kWave) {
        const int i = base + lane;
        const bool in = i < active0;
        const uint32_t a = in ? c.sa[i] : 0u, b = in ? c.sb[i] : 0u;
        const uint32_t q = (P.track_ids && in) ? c.sq[i] : 0u;
        const bool vic = in && rec_on_link<R32>(P, a, link), sur = in && !vic;
        const uint64_t bv = __ballot(vic), bs = __ballot(sur);
        wave_sync();                                                        // the chunk is read before a survivor lands in it
        if (vic) {
            const int j = nv + __popcll((unsigned long long)(bv & lanes_below(lane)));
            vsa[j] = a; vsb[j] = b; vidx[j] = (uint16_t)i;
            if (P.track_ids) vsq[j] = q;
        }
        if (sur) {
            const int j = ns + __popcll((unsigned long long)(bs & lanes_below(lane)));   // <= i
            c.sa[j] = a; c.sb[j] = b;
            if (P.track_ids) c.sq[j] = q;
        }
        nv += __popcll((unsigned long long)bv);
        ns += __popcll((unsigned long long)bs);
    }
    c.active = ns;
    wave_sync();

    // ---- 2. all victims leave at once (_release_path: n + 1 slots, clamped at S)
    for (int j = 0; j < nv; j++) {
        const uint32_t a = (uint32_t)uniform_i32((int)vsa[j]), b = (uint32_t)uniform_i32((int)vsb[j]);
        const int sk = rec_slot<R32>(a, b), nk = rec_n<R32>(a, b);
        if (R32) mark_mask(c, a, sk, sk + nk + 1, true);
        else {
            const int pk = a & 0xFFFF;
            const int hops = G(P.path_hops)[pk];
            const int mylink = (lane < hops) ? G(P.path_links)[pk * P.max_hops + lane] : 0;
            mark_links(c, hops, mylink, sk, sk + nk + 1, true);
        }
    }

    // ---- 3. restoration, one victim after the other
    int vcap = 0, restored = 0, rcap = 0, lost_ns = 0, lost_qot = 0, xhops = 0, xslots = 0;
    double low = INFINITY;
    for (int j = 0; j < nv; j++) {
        const uint32_t a = (uint32_t)uniform_i32((int)vsa[j]), b = (uint32_t)uniform_i32((int)vsb[j]);
        const int old_path = rec_path<R32>(a, b), n = rec_n<R32>(a, b), m = rec_mod<R32>(a, b);
        const int cap = n * P.mod_se[m], old_hops = uniform_i32(G(P.path_hops)[old_path]);
        const int pair = uniform_i32(G(path_pair)[old_path]);
        vcap += cap;
        c.skip_id = P.track_ids ? uniform_i32((int)vsq[j]) : -1;            // its namesakes are no interferers (quirk Q12)
        bool found = false, refused = false;
        int action = K * M * S;
        for (int k = 0; k < K && pair >= 0 && !found; k++) {
            const int path = uniform_i32(G(P.pair_paths)[pair * K + k]);
            if (path < 0) break;
            const PathRef p = load_path(c, path);
            if (uniform_i32((int)(((link < 64 ? p.m0 >> link : p.m1 >> (link - 64)) & 1ull)))) continue;   // crosses the failed link
            uint64_t runs = path_free_ext(c, p);
            int r = 1, L = -1;
            for (int mm = M - 1; mm >= 0; mm--) {
                const int nn = failure_slots(cap, P.mod_se[mm]);
                if (nn > S) continue;
                if (nn + 1 < r) { runs = path_free_ext(c, p); r = 1; }
                runs = run_and(runs, r, nn + 1);
                const int first = first_set(runs);
                if (first < 0) continue;
                const GnCoef kf = coef_for_slots(c, nn);
                if (P.ase_shortcut) {                                       // exact lower bound, see policy_first_fit
                    const double bw = P.slot_bw * nn;
                    const double fc = P.f0 + (P.slot_bw * first) + (P.slot_bw * (nn / 2.0));
                    double lb = (bw * fc * p.ase) * c.rp[0];
                    if (UA) lb += kf.nlic * (p.w1 * kf.selfa);
                    if (uniform_i32(lb >= c.lim[mm] * (1.0 + kQotBand))) { refused = true; continue; }
                }
                if (L < 0) L = gn_build_list<R32>(c, p.m0, p.m1);
                const GnLin g = gn_eval<UA, R32>(c, p, L, first, nn, kf);
                if (!qot_ok(c, g, mm, margin)) { refused = true; continue; }
                // provisioned as the step provisions, appended as the step appends an accept
                int end = first + nn;
                if (end < S) end += 1;
                mark_links<false>(c, p.hops, p.mylink, first, end, false);
                if (lane == 0) {
                    uint32_t ra, rb;
                    rec_pack<R32>(path, p.m0, first, nn, mm, ra, rb);
                    c.sa[c.active] = ra; c.sb[c.active] = rb;               // active < active0 <= C: this victim's place is free
                    if (P.track_ids) c.sq[c.active] = vsq[j];
                }
                c.active++;
                wave_sync();
                found = true;
                action = k * M * S + (M - 1 - mm) * S + first;
                restored++;
                rcap += cap;
                xhops += uniform_i32(p.hops) - old_hops;
                xslots += nn * uniform_i32(p.hops) - n * old_hops;
                low = fmin(low, -10.0 * log10(uniform_f64(g.ase) + uniform_f64(g.nli)) - P.mod_thr[mm] - margin);
                break;
            }
        }
        if (!found) { if (refused) lost_qot++; else lost_ns++; }
        if (srow && lane == 0) srow[vidx[j]] = action;
    }
    if (lane < kFailureImpact) {
        const double v[kFailureImpact] = {0.0, (double)nv, (double)vcap, (double)restored, (double)rcap, (double)lost_ns,
                                          (double)lost_qot, (double)xhops, (double)xslots, restored ? low : NAN};
        double r = v[0];
        for (int k = 1; k < kFailureImpact; k++) r = lane == k ? v[k] : r;
        o[lane] = r;
    }
}

// ---- link sets (ongym_failure_sets): two links at once, a node (all its links), a shared-risk link group ----------------------
// k_failure_sets is k_failure_impact with the failed link replaced by a set of links, two wave-uniform mask words f0 / f1 in the
// bit order of the path masks, loaded once per scenario.  Two tests differ: a record is a victim if its route's mask meets
// the set, a route is eligible if its mask does not; and the row has two more columns (lost_no_route, failed_links).  Same LDS
// layout (failure_lds_bytes), same loop bounds.  It is a kernel of its own, not a second instantiation of one templated body:
// with the body shared, k_failure_impact kept its VGPRs and occupancy but spilled 26-28 SGPRs instead of 18-20.
constexpr int kFailureSets = ONGYM_N_FAILURE_SETS;        // set_out doubles per (replica, link set): link_out's ten, lost_no_route, failed_links
constexpr int kMaxFailureSets = ONGYM_MAX_FAILURE_SETS;   // link sets per replica: the grid's y extent

// a set is evaluated if it is not empty and has no bit at an index >= E
__device__ __forceinline__ bool failure_set_valid(int E, uint64_t f0, uint64_t f1) {
    const uint64_t v0 = E >= 64 ? ~0ull : (1ull << E) - 1, v1 = E >= 128 ? ~0ull : E > 64 ? (1ull << (E - 64)) - 1 : 0ull;
    return (f0 | f1) != 0 && ((f0 & ~v0) | (f1 & ~v1)) == 0;
}

template <bool R32>
__device__ __forceinline__ bool rec_on_set(const Params &P, uint32_t a, uint64_t f0, uint64_t f1) {
    if (R32) return (a & (uint32_t)f0) != 0;                                // a valid set with E <= 32 lies in f0's low word
    const int p = (int)(a & 0xFFFF);
    return ((G(P.path_mask)[2 * p] & f0) | (G(P.path_mask)[2 * p + 1] & f1)) != 0;
}

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    return (uint32_t)uniform_i32((int)(uint32_t)v) | ((uint64_t)(uint32_t)uniform_i32((int)(v >> 32)) << 32);
}

// sets: uint64 [batch][F][2] (per_replica) or [F][2] (one list for every replica)
template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_failure_sets(const Params *__restrict__ Pp, int F, const uint64_t *__restrict__ sets,
                                                     int per_replica, const int32_t *__restrict__ path_pair,
                                                     double *__restrict__ set_out, int32_t *__restrict__ svc_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    const int C = P.capacity, K = P.k_paths, M = P.n_mods, S = P.n_slots, lane = c.lane, f = blockIdx.y;
    uint32_t *vsb = reinterpret_cast<uint32_t *>(smem + lds_bytes(P));
    uint32_t *vsq = P.track_ids ? vsb + C : nullptr;                        // without id tracking vidx lies there
    uint16_t *vidx = reinterpret_cast<uint16_t *>(vsb + (P.track_ids ? 2 : 1) * (size_t)C);
    const size_t col = (size_t)c.replica * F + f;
    double *o = set_out + col * kFailureSets;
    int32_t *srow = svc_out ? svc_out + col * C : nullptr;
    const size_t at = 2 * (per_replica ? col : (size_t)f);
    const uint64_t f0 = uniform_u64(G(sets)[at]), f1 = uniform_u64(G(sets)[at + 1]);
    if (srow) {
        for (int i = lane; i < C; i += kWave) srow[i] = -1;
        __threadfence();                                                    // the victims' entries are stored over these below
    }
    if (!failure_set_valid(P.n_links, f0, f1)) {
        if (lane < kFailureSets) o[lane] = lane == 0 ? 1.0 : NAN;
        return;
    }
    load_state(c);
    uint32_t *vsa = reinterpret_cast<uint32_t *>(c.sr);                     // (load_state's wave_sync orders its stores to `sr`)
    const double margin = c.e->margin;

    // ---- 1. victims (a route that meets the set: each record once) to the saved list, survivors moved down, in record order
    const int active0 = c.active;
    int nv = 0, ns = 0;
    for (int base = 0; base < active0; base += kWave) {
        const int i = base + lane;
        const bool in = i < active0;
        const uint32_t a = in ? c.sa[i] : 0u, b = in ? c.sb[i] : 0u;
        const uint32_t q = (P.track_ids && in) ? c.sq[i] : 0u;
        const bool vic = in && rec_on_set<R32>(P, a, f0, f1), sur = in && !vic;
        const uint64_t bv = __ballot(vic), bs = __ballot(sur);
        wave_sync();                                                        // the chunk is read before a survivor lands in it
        if (vic) {
            const int j = nv + __popcll((unsigned long long)(bv & lanes_below(lane)));
            vsa[j] = a; vsb[j] = b; vidx[j] = (uint16_t)i;
            if (P.track_ids) vsq[j] = q;
        }
        if (sur) {
            const int j = ns + __popcll((unsigned long long)(bs & lanes_below(lane)));   // <= i
            c.sa[j] = a; c.sb[j] = b;
            if (P.track_ids) c.sq[j] = q;
        }
        nv += __popcll((unsigned long long)bv);
        ns += __popcll((unsigned long long)bs);
    }
    c.active = ns;
    wave_sync();

    // ---- 2. all victims leave at once (_release_path: n + 1 slots, clamped at S)
    for (int j = 0; j < nv; j++) {
        const uint32_t a = (uint32_t)uniform_i32((int)vsa[j]), b = (uint32_t)uniform_i32((int)vsb[j]);
        const int sk = rec_slot<R32>(a, b), nk = rec_n<R32>(a, b);
        if (R32) mark_mask(c, a, sk, sk + nk + 1, true);
        else {
            const int pk = a & 0xFFFF;
            const int hops = G(P.path_hops)[pk];
            const int mylink = (lane < hops) ? G(P.path_links)[pk * P.max_hops + lane] : 0;
            mark_links(c, hops, mylink, sk, sk + nk + 1, true);
        }
    }

    // ---- 3. restoration, one victim after the other, over the routes that meet no failed link
    int vcap = 0, restored = 0, rcap = 0, lost_ns = 0, lost_qot = 0, lost_nr = 0, xhops = 0, xslots = 0;
    double low = INFINITY;
    for (int j = 0; j < nv; j++) {
        const uint32_t a = (uint32_t)uniform_i32((int)vsa[j]), b = (uint32_t)uniform_i32((int)vsb[j]);
        const int old_path = rec_path<R32>(a, b), n = rec_n<R32>(a, b), m = rec_mod<R32>(a, b);
        const int cap = n * P.mod_se[m], old_hops = uniform_i32(G(P.path_hops)[old_path]);
        const int pair = uniform_i32(G(path_pair)[old_path]);
        vcap += cap;
        c.skip_id = P.track_ids ? uniform_i32((int)vsq[j]) : -1;            // its namesakes are no interferers (quirk Q12)
        bool found = false, refused = false, any_route = false;
        int action = K * M * S;
        for (int k = 0; k < K && pair >= 0 && !found; k++) {
            const int path = uniform_i32(G(P.pair_paths)[pair * K + k]);
            if (path < 0) break;
            const PathRef p = load_path(c, path);
            if (uniform_i32((int)(((p.m0 & f0) | (p.m1 & f1)) != 0))) continue;   // crosses a failed link
            any_route = true;
            uint64_t runs = path_free_ext(c, p);
            int r = 1, L = -1;
            for (int mm = M - 1; mm >= 0; mm--) {
                const int nn = failure_slots(cap, P.mod_se[mm]);
                if (nn > S) continue;
                if (nn + 1 < r) { runs = path_free_ext(c, p); r = 1; }
                runs = run_and(runs, r, nn + 1);
                const int first = first_set(runs);
                if (first < 0) continue;
                const GnCoef kf = coef_for_slots(c, nn);
                if (P.ase_shortcut) {                                       // exact lower bound, see policy_first_fit
                    const double bw = P.slot_bw * nn;
                    const double fc = P.f0 + (P.slot_bw * first) + (P.slot_bw * (nn / 2.0));
                    double lb = (bw * fc * p.ase) * c.rp[0];
                    if (UA) lb += kf.nlic * (p.w1 * kf.selfa);
                    if (uniform_i32(lb >= c.lim[mm] * (1.0 + kQotBand))) { refused = true; continue; }
                }
                if (L < 0) L = gn_build_list<R32>(c, p.m0, p.m1);
                const GnLin g = gn_eval<UA, R32>(c, p, L, first, nn, kf);
                if (!qot_ok(c, g, mm, margin)) { refused = true; continue; }
                // provisioned as the step provisions, appended as the step appends an accept
                int end = first + nn;
                if (end < S) end += 1;
                mark_links<false>(c, p.hops, p.mylink, first, end, false);
                if (lane == 0) {
                    uint32_t ra, rb;
                    rec_pack<R32>(path, p.m0, first, nn, mm, ra, rb);
                    c.sa[c.active] = ra; c.sb[c.active] = rb;               // active < active0 <= C: this victim's place is free
                    if (P.track_ids) c.sq[c.active] = vsq[j];
                }
                c.active++;
                wave_sync();
                found = true;
                action = k * M * S + (M - 1 - mm) * S + first;
                restored++;
                rcap += cap;
                xhops += uniform_i32(p.hops) - old_hops;
                xslots += nn * uniform_i32(p.hops) - n * old_hops;
                low = fmin(low, -10.0 * log10(uniform_f64(g.ase) + uniform_f64(g.nli)) - P.mod_thr[mm] - margin);
                break;
            }
        }
        if (!found) { if (refused) lost_qot++; else lost_ns++; }
        if (!any_route) lost_nr++;                                          // no route of its node pair is left at all
        if (srow && lane == 0) srow[vidx[j]] = action;
    }
    if (lane < kFailureSets) {
        const double v[kFailureSets] = {0.0, (double)nv, (double)vcap, (double)restored, (double)rcap, (double)lost_ns,
                                        (double)lost_qot, (double)xhops, (double)xslots, restored ? low : NAN, (double)lost_nr,
                                        (double)(__popcll((unsigned long long)f0) + __popcll((unsigned long long)f1))};
        double r = v[0];
        for (int k = 1; k < kFailureSets; k++) r = lane == k ? v[k] : r;
        o[lane] = r;
    }
}

}  // namespace ongym
