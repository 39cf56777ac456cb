// ongym_cut.hpp — link failures on LIVE replicas (ongym_cut_links, ongym_repair_links, ongym_failed_links, include/ongym.h).
// ongym_failure_sets answers "what if" on a private copy; these calls change the replica itself, so that traffic continues on the
// degraded network and the fibre can be returned later.
//
// A failed link is a row of the bitmap without a free slot in [0, S) that no running record crosses.  Nothing else is stored:
// every step kernel, policy, observation and mask sees a full link and places nothing on it, no release ever touches the row
// (releases walk a record's own route), and save / load / fork carry it with the bitmap.  Repair sets the row's bits again.
// The rule is exact as long as the bitmap is the union of the records' provisioned ranges.
//
// k_cut_links: one wavefront per replica, grid (batch), on the step kernels' set-up (Ctx, load_state).  Its body is
// k_failure_sets' three phases (ongym_failure.hpp) with one link set per replica and two differences:
//   (a) it keeps everything a record owns: the saved victim list also carries the release time (with its sign, the disrupted
//       flag of measure_disruptions) and, with id tracking, the id and Service.OSNR; survivors move down with theirs, a restored
//       victim is appended with its own release time and id
//   (b) after restoration it clears [0, S) of every failed row, zeroes the launch's work counters (so that store_state adds
//       nothing to total_*) and stores the state back.
// A replica whose set is empty or has a bit at an index >= E returns before load_state: it is left byte for byte as it was.
// Every loop is bounded by `active`, K, M, E or the row words.
//
// LDS: the state block | (vso f64[C] with id tracking) | vsa u32[C] | vsb u32[C] | vsr f32[C] | (vsq u32[C]) | vidx u16[C].
// NSFNET-320, C = 448: 8 208 + 6 272 = 14 480 B, twelve 1 280-byte granules, 10 replicas per CU.
//
// k_repair_links and k_failed_links: one wavefront per replica, no LDS.  Both OR the route masks of the running records and test
// every row for a free bit in [0, S); lane l owns links l and l + 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_failure.hpp"

namespace ongym {

constexpr int kCutLinks = ONGYM_N_CUT_LINKS;   // cut_out doubles per replica: set_out's twelve, dropped

__host__ __device__ inline size_t cut_lds_bytes(const Params &P) {
    return (lds_bytes(P) + (size_t)P.capacity * (P.track_ids ? 26 : 14) + 15) & ~(size_t)15;
}

// sets: uint64 [batch][2] (per_replica) or [2] (one set for every replica)
template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_cut_links(const Params *__restrict__ Pp, const uint64_t *__restrict__ sets, int per_replica,
                                                  int no_restore, const int32_t *__restrict__ path_pair,
                                                  double *__restrict__ cut_out, int32_t *__restrict__ svc_out,
                                                  int32_t *__restrict__ index_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    const int C = P.capacity, K = P.k_paths, M = P.n_mods, S = P.n_slots, lane = c.lane;
    double *vso = reinterpret_cast<double *>(smem + lds_bytes(P));         // lds_bytes is a multiple of 16
    uint32_t *vsa = reinterpret_cast<uint32_t *>(vso + (P.track_ids ? C : 0));
    uint32_t *vsb = vsa + C;
    float *vsr = reinterpret_cast<float *>(vsb + C);
    uint32_t *vsq = reinterpret_cast<uint32_t *>(vsr + C);                 // without id tracking vidx lies there
    uint16_t *vidx = reinterpret_cast<uint16_t *>(vsq + (P.track_ids ? C : 0));
    double *o = cut_out + (size_t)c.replica * kCutLinks;
    int32_t *srow = svc_out ? svc_out + (size_t)c.replica * C : nullptr;
    int32_t *irow = index_out ? index_out + (size_t)c.replica * C : nullptr;
    const size_t at = per_replica ? 2 * (size_t)c.replica : 0;
    const uint64_t f0 = uniform_u64(G(sets)[at]), f1 = uniform_u64(G(sets)[at + 1]);
    if (srow || irow) {
        for (int i = lane; i < C; i += kWave) {
            if (srow) srow[i] = -1;
            if (irow) irow[i] = -1;
        }
        __threadfence();                                                    // lane 0 stores the victims' entries over these below
    }
    if (!failure_set_valid(P.n_links, f0, f1)) {
        if (lane < kCutLinks) o[lane] = lane == 0 ? 1.0 : NAN;
        return;                                                             // before any store to the replica
    }
    load_state(c);
    const double margin = c.e->margin;

    // ---- 1. victims to the saved list, survivors moved down, both in record order and with everything they own
    const int active0 = c.active;
    int nv = 0, ns = 0;
    for (int base = 0; base < active0; base += kWave) {
        const int i = base + lane;
        const bool in = i < active0;
        const uint32_t a = in ? c.sa[i] : 0u, b = in ? c.sb[i] : 0u;
        const float r = in ? c.sr[i] : 0.f;
        const uint32_t q = (P.track_ids && in) ? c.sq[i] : 0u;
        const double so = (P.track_ids && in) ? c.so[i] : 0.0;
        const bool vic = in && rec_on_set<R32>(P, a, f0, f1), sur = in && !vic;
        const uint64_t bv = __ballot(vic), bs = __ballot(sur);
        wave_sync();                                                        // the chunk is read before a survivor lands in it
        if (vic) {
            const int j = nv + __popcll((unsigned long long)(bv & lanes_below(lane)));
            vsa[j] = a; vsb[j] = b; vsr[j] = r; vidx[j] = (uint16_t)i;
            if (P.track_ids) { vsq[j] = q; vso[j] = so; }
        }
        if (sur) {
            const int j = ns + __popcll((unsigned long long)(bs & lanes_below(lane)));   // <= i
            c.sa[j] = a; c.sb[j] = b; c.sr[j] = r;
            if (P.track_ids) { c.sq[j] = q; c.so[j] = so; }
            if (irow) irow[i] = j;                                          // this lane initialised entry i itself
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

    // ---- 3. restoration, one victim after the other, over the routes that meet no failed link (skipped with no_restore)
    int vcap = 0, restored = 0, rcap = 0, lost_ns = 0, lost_qot = 0, lost_nr = 0, xhops = 0, xslots = 0;
    double low = INFINITY;
    for (int j = 0; j < nv; j++) {
        const uint32_t a = (uint32_t)uniform_i32((int)vsa[j]), b = (uint32_t)uniform_i32((int)vsb[j]);
        const int old_path = rec_path<R32>(a, b), n = rec_n<R32>(a, b), m = rec_mod<R32>(a, b);
        const int cap = n * P.mod_se[m];
        vcap += cap;
        if (no_restore) {                                                   // dropped: it leaves as a departure leaves
            if (srow && lane == 0) srow[vidx[j]] = K * M * S;
            continue;
        }
        const int old_hops = uniform_i32(G(P.path_hops)[old_path]);
        const int pair = uniform_i32(G(path_pair)[old_path]);
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
                // provisioned as the step provisions, appended as the step appends an accept, with what the victim owned
                int end = first + nn;
                if (end < S) end += 1;
                mark_links<false>(c, p.hops, p.mylink, first, end, false);
                const double osnr = -10.0 * log10(uniform_f64(g.ase) + uniform_f64(g.nli));
                if (lane == 0) {
                    uint32_t ra, rb;
                    rec_pack<R32>(path, p.m0, first, nn, mm, ra, rb);
                    c.sa[c.active] = ra; c.sb[c.active] = rb;               // active < active0 <= C: this victim's place is free
                    c.sr[c.active] = vsr[j];
                    if (P.track_ids) {
                        c.sq[c.active] = vsq[j];
                        c.e->osnr_flushed += osnr - vso[j];                 // the Service object is updated, as defragment() does
                        c.so[c.active] = osnr;
                    }
                    if (irow) irow[vidx[j]] = c.active;
                }
                c.active++;
                wave_sync();
                found = true;
                action = k * M * S + (M - 1 - mm) * S + first;
                restored++;
                rcap += cap;
                xhops += uniform_i32(p.hops) - old_hops;
                xslots += nn * uniform_i32(p.hops) - n * old_hops;
                low = fmin(low, osnr - P.mod_thr[mm] - margin);
                break;
            }
        }
        if (!found) { if (refused) lost_qot++; else lost_ns++; }
        if (!any_route) lost_nr++;                                          // no route of its node pair is left at all
        if (srow && lane == 0) srow[vidx[j]] = action;
    }

    // ---- 4. the failed rows lose every free slot of [0, S) (bits at and above S stay), and the state goes back
    for (int l = lane; l < P.n_links; l += kWave) {
        if (!(((l < 64 ? f0 >> l : f1 >> (l - 64)) & 1ull))) continue;
        for (int w = 0; w < P.row_words; w++) c.occ[l * P.row_words + w] &= ~word_range(w, 0, S);
    }
    wave_sync();
    c.lane_terms = 0; c.gn_evals = 0; c.gn_skips = 0;                       // a cut is no step: total_* stay
    c.paths_tried = 0; c.path_hops = 0; c.active_sum = 0;
    c.skip_id = -1;
    store_state(c);

    if (lane < kCutLinks) {
        const double v[kCutLinks] = {0.0, (double)nv, (double)vcap, (double)restored, (double)rcap, (double)lost_ns,
                                     (double)lost_qot, (double)xhops, (double)xslots, restored ? low : NAN, (double)lost_nr,
                                     (double)(__popcll((unsigned long long)f0) + __popcll((unsigned long long)f1)),
                                     no_restore ? (double)nv : 0.0};
        double r = v[0];
        for (int k = 1; k < kCutLinks; k++) r = lane == k ? v[k] : r;
        o[lane] = r;
    }
}

// ---- repair and query ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v) {
    int lo = (int)(uint32_t)v, hi = (int)(v >> 32);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { lo |= __shfl_xor(lo, m); hi |= __shfl_xor(hi, m); }
    return (uint32_t)lo | ((uint64_t)(uint32_t)hi << 32);
}

// The failed links of a replica as two mask words, read from the stored state: row e has no free slot in [0, S) and no running
// record's route contains e.
template <bool R32>
__device__ __forceinline__ void failed_masks(const Params &P, int replica, int lane, uint64_t &d0, uint64_t &d1) {
    const int active = uniform_i32(P.env[replica].st.active);
    const size_t off = (size_t)replica * P.capacity;
    uint64_t u0 = 0, u1 = 0;                                                // links that records cross
    for (int i = lane; i < active; i += kWave) {
        const uint32_t a = P.svc_a[off + i];
        if (R32) u0 |= a;
        else { const int p = (int)(a & 0xFFFF); u0 |= G(P.path_mask)[2 * p]; u1 |= G(P.path_mask)[2 * p + 1]; }
    }
    u0 = wave_or_u64(u0); u1 = wave_or_u64(u1);
    const uint64_t *g = P.occ + (size_t)replica * P.n_links * P.row_words;
    bool full[2];
    for (int h = 0; h < 2; h++) {
        const int l = lane + 64 * h;
        uint64_t any = 0;
        if (l < P.n_links)
            for (int w = 0; w < P.row_words; w++) any |= g[(size_t)l * P.row_words + w] & word_range(w, 0, P.n_slots);
        full[h] = l < P.n_links && any == 0;
    }
    d0 = __ballot(full[0]) & ~u0;
    d1 = __ballot(full[1]) & ~u1;
}

template <bool R32>
__global__ __launch_bounds__(64) void k_failed_links(const Params *__restrict__ Pp, uint64_t *__restrict__ failed_out) {
    const Params &P = *Pp;
    const int lane = threadIdx.x, replica = blockIdx.x;
    uint64_t d0, d1;
    failed_masks<R32>(P, replica, lane, d0, d1);
    if (lane < 2) failed_out[2 * (size_t)replica + lane] = lane ? d1 : d0;
}

// sets as k_cut_links'.  The links of the set that are failed get [0, S) of their rows back; the others are ignored.
template <bool R32>
__global__ __launch_bounds__(64) void k_repair_links(const Params *__restrict__ Pp, const uint64_t *__restrict__ sets,
                                                     int per_replica, int32_t *__restrict__ repaired_out) {
    const Params &P = *Pp;
    const int lane = threadIdx.x, replica = blockIdx.x;
    const size_t at = per_replica ? 2 * (size_t)replica : 0;
    const uint64_t f0 = uniform_u64(G(sets)[at]), f1 = uniform_u64(G(sets)[at + 1]);
    uint64_t d0, d1;
    failed_masks<R32>(P, replica, lane, d0, d1);
    d0 &= f0; d1 &= f1;
    uint64_t *g = P.occ + (size_t)replica * P.n_links * P.row_words;
    for (int h = 0; h < 2; h++) {
        const int l = lane + 64 * h;
        if (l >= P.n_links || !(((h ? d1 : d0) >> lane) & 1ull)) continue;
        for (int w = 0; w < P.row_words; w++) g[(size_t)l * P.row_words + w] |= word_range(w, 0, P.n_slots);
    }
    if (repaired_out && lane == 0) repaired_out[replica] = __popcll((unsigned long long)d0) + __popcll((unsigned long long)d1);
}

}  // namespace ongym
