// ongym_move.hpp — moving running lightpaths on LIVE replicas (ongym_move_services, include/ongym.h): a chosen record is placed
// again, at a chosen action of its node pair's routes or where first fit puts it, and keeps its index, release time and id.
//
// A move is a restoration (ongym_cut.hpp, phase 3) of ONE record with no failed link, written back to the record's own index:
// its spectrum counts as free, it is no interferer of its own evaluation (nor are its namesakes under id tracking, quirk Q12),
// and the new place passes the step's admission test: a candidate start of `_get_candidates` for the new slot count, the exact
// ASE lower bound where first fit uses it, gn_build_list / gn_eval / qot_ok with the replica's margin.
//
// k_move_services: one wavefront per replica, grid (batch), on the step kernels' set-up (Ctx, load_state).  The moves of a replica
// run one after the other (wave-uniform loop), each on the state the previous one left:
//   1. resolve the record: an index, or ONGYM_MOVE_TOP = the highest last slot among the records no move of this call has
//      attempted (lanes over records, one wave-wide max of a packed key); every resolved record is marked attempted
//   2. release its range as a departure does (n + 1 slots, clamped at S)
//   3. explicit target: `start` must be a candidate start on the target route; first fit: the restorations' search over the
//      pair's routes (or the record's own route only).  A format under which the service would take more than max_slots
//      slots is no spectrum for an explicit target and is passed over by first fit: the lean step kernels index their pair
//      table and build their release masks on the traffic table's widest slot count, and traffic goes on after a move.  The record stays where it is in the arrays: gn_build_list<R32, true>
//      leaves index `idx` out of the interferer list, so no record changes place.
//   4. moved: provision the new range, rewrite the record words in place (and Service.OSNR, osnr_flushed with ids).  Otherwise
//      provision the old range again: the bitmap is the union of the records' ranges, so this is the row as
//      it was.
// A replica none of whose moves succeeds stores nothing: it is left byte for byte as it was.  Otherwise the launch's work
// counters are zeroed before store_state, as the cut does, so no total_* changes.
// Every loop is bounded by n_moves, `active`, K, M, E or the row words.
//
// LDS: the state block | attempted bits u32[C / 32].  NSFNET-320, C = 448: 8 208 + 56 = 8 264 B, seven 1 280-byte granules.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_failure.hpp"

namespace ongym {

constexpr int kMoveOut = ONGYM_N_MOVE_COLUMNS;   // move_out doubles per (replica, move)

__host__ __device__ inline size_t move_lds_bytes(const Params &P) {
    return (lds_bytes(P) + (size_t)P.capacity / 8 + 15) & ~(size_t)15;      // capacity % 64 == 0
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        uint64_t o = __shfl_xor((unsigned long long)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// the range [lo, hi) of a record's route set free or occupied, as the step kernels release a departure
template <bool R32>
__device__ __forceinline__ void move_mark_record(Ctx &c, uint32_t a, int lo, int hi, bool free_) {
    const Params &P = c.P;
    if (R32) mark_mask(c, a, lo, hi, free_);
    else {
        const int pk = a & 0xFFFF;
        const int hops = G(P.path_hops)[pk];
        const int mylink = (c.lane < hops) ? G(P.path_links)[pk * P.max_hops + c.lane] : 0;
        mark_links(c, hops, mylink, lo, hi, free_);
    }
}

// moves: int32 [batch][n_moves][2] = (record, target).  max_slots: the widest record a move may write (<= S): what the lean step
// kernels of this environment can carry, S where none will ever run (ongym_move_services, ongym_hip.hip)
template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_move_services(const Params *__restrict__ Pp, int n_moves, const int32_t *__restrict__ moves,
                                                      int own_route, int max_slots, const int32_t *__restrict__ path_pair,
                                                      double *__restrict__ move_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    const int C = P.capacity, K = P.k_paths, M = P.n_mods, S = P.n_slots, lane = c.lane;
    uint32_t *att = reinterpret_cast<uint32_t *>(smem + lds_bytes(P));      // lds_bytes is a multiple of 16
    for (int i = lane; i < C / 32; i += kWave) att[i] = 0u;
    load_state(c);                                                          // (its wave_sync orders the stores to `att`)
    const double margin = c.e->margin;
    const int32_t *mrow = moves + (size_t)c.replica * n_moves * 2;
    double *orow = move_out + (size_t)c.replica * n_moves * kMoveOut;
    int moved = 0;

    for (int t = 0; t < n_moves; t++) {
        const int sel = uniform_i32(G(mrow)[2 * t]), target = uniform_i32(G(mrow)[2 * t + 1]);
        int status = 1, idx = -1, old_action = -1, new_action = -1, delta = 0;
        double mrg = NAN;
        do {
            // ---- 1. the record
            if (sel == ONGYM_MOVE_TOP) {
                uint64_t key = 0;                                           // (last slot + 1) << 16 | (0xFFFF - record index)
                for (int i = lane; i < c.active; i += kWave) {
                    if ((att[i >> 5] >> (i & 31)) & 1u) continue;
                    const uint32_t a = c.sa[i], b = c.sb[i];
                    const uint64_t k = ((uint64_t)(rec_slot<R32>(a, b) + rec_n<R32>(a, b)) << 16) | (uint64_t)(0xFFFF - i);
                    key = k > key ? k : key;
                }
                key = wave_max_u64(key);
                if (key == 0) break;                                        // no record left
                idx = uniform_i32(0xFFFF - (int)(key & 0xFFFF));
            } else {
                if (sel < 0 || sel >= c.active) break;
                idx = sel;
            }
            if (lane == 0) att[idx >> 5] |= 1u << (idx & 31);
            wave_sync();
            const uint32_t a = (uint32_t)uniform_i32((int)c.sa[idx]), b = (uint32_t)uniform_i32((int)c.sb[idx]);
            const int old_path = rec_path<R32>(a, b), s = rec_slot<R32>(a, b), n = rec_n<R32>(a, b), m = rec_mod<R32>(a, b);
            const int cap = n * P.mod_se[m];
            const int pair = uniform_i32(G(path_pair)[old_path]);
            if (pair < 0) { idx = -1; break; }                              // (no such record passes the call's refusals)
            int old_k = -1;
            for (int k = K - 1; k >= 0; k--)
                if (uniform_i32(G(P.pair_paths)[pair * K + k]) == old_path) old_k = k;
            if (old_k < 0) { idx = -1; break; }
            old_action = new_action = old_k * M * S + (M - 1 - m) * S + s;
            const int old_hops = uniform_i32(G(P.path_hops)[old_path]);

            // ---- the target of an explicit move
            int tk = -1, tm = -1, ts = -1, tn = 0, tpath = -1;
            if (target != ONGYM_MOVE_FIRST_FIT) {
                if (target < 0 || target >= K * M * S) break;
                tk = target / (M * S); tm = M - 1 - (target / S) % M; ts = target % S;
                tpath = uniform_i32(G(P.pair_paths)[pair * K + tk]);
                if (tpath < 0) break;
                if (tpath == old_path && tm == m && ts == s) { status = 2; break; }
                tn = failure_slots(cap, P.mod_se[tm]);
                if (tn > max_slots) { status = 3; break; }
            }

            // ---- 2. its own spectrum counts as free (_release_path: n + 1 slots, clamped at S)
            move_mark_record<R32>(c, a, s, s + n + 1, true);
            c.skip_id = P.track_ids ? uniform_i32((int)c.sq[idx]) : -1;     // its namesakes are no interferers (quirk Q12)

            // ---- 3. the new place
            bool found = false, refused = false;
            int nk = -1, nm = -1, ns = -1, nn = 0, npath = -1, nhops = 0, nmylink = 0;
            uint64_t nm0 = 0;
            double osnr = 0.0;
            if (target != ONGYM_MOVE_FIRST_FIT) {
                const PathRef p = load_path(c, tpath);
                int r = 1;
                const uint64_t runs = run_and(path_free_ext(c, p), r, tn + 1);
                const bool cand = __ballot(lane == (ts >> 6) && ((runs >> (ts & 63)) & 1ull)) != 0;
                if (cand) {
                    const GnCoef kf = coef_for_slots(c, tn);
                    bool bound = false;
                    if (P.ase_shortcut) {                                   // exact lower bound, see policy_first_fit
                        const double bw = P.slot_bw * tn;
                        const double fc = P.f0 + (P.slot_bw * ts) + (P.slot_bw * (tn / 2.0));
                        double lb = (bw * fc * p.ase) * c.rp[0];
                        if (UA) lb += kf.nlic * (p.w1 * kf.selfa);
                        bound = uniform_i32(lb >= c.lim[tm] * (1.0 + kQotBand)) != 0;
                    }
                    if (bound) refused = true;
                    else {
                        const int L = gn_build_list<R32, true>(c, p.m0, p.m1, idx);
                        const GnLin g = gn_eval<UA, R32>(c, p, L, ts, tn, kf);
                        if (!qot_ok(c, g, tm, margin)) refused = true;
                        else {
                            found = true;
                            nk = tk; nm = tm; ns = ts; nn = tn; npath = tpath;
                            nhops = p.hops; nmylink = p.mylink; nm0 = p.m0;
                            osnr = -10.0 * log10(uniform_f64(g.ase) + uniform_f64(g.nli));
                        }
                    }
                }
            } else {
                // first fit's search, a restoration of k_cut_links with an empty failed set
                for (int k = own_route ? old_k : 0; k < (own_route ? old_k + 1 : K) && !found; k++) {
                    const int path = uniform_i32(G(P.pair_paths)[pair * K + k]);
                    if (path < 0) break;
                    const PathRef p = load_path(c, path);
                    uint64_t runs = path_free_ext(c, p);
                    int r = 1, L = -1;
                    for (int mm = M - 1; mm >= 0; mm--) {
                        const int fn = failure_slots(cap, P.mod_se[mm]);
                        if (fn > max_slots) continue;
                        if (fn + 1 < r) { runs = path_free_ext(c, p); r = 1; }
                        runs = run_and(runs, r, fn + 1);
                        const int first = first_set(runs);
                        if (first < 0) continue;
                        const GnCoef kf = coef_for_slots(c, fn);
                        if (P.ase_shortcut) {                               // exact lower bound, see policy_first_fit
                            const double bw = P.slot_bw * fn;
                            const double fc = P.f0 + (P.slot_bw * first) + (P.slot_bw * (fn / 2.0));
                            double lb = (bw * fc * p.ase) * c.rp[0];
                            if (UA) lb += kf.nlic * (p.w1 * kf.selfa);
                            if (uniform_i32(lb >= c.lim[mm] * (1.0 + kQotBand))) { refused = true; continue; }
                        }
                        if (L < 0) L = gn_build_list<R32, true>(c, p.m0, p.m1, idx);
                        const GnLin g = gn_eval<UA, R32>(c, p, L, first, fn, kf);
                        if (!qot_ok(c, g, mm, margin)) { refused = true; continue; }
                        found = true;
                        nk = k; nm = mm; ns = first; nn = fn; npath = path;
                        nhops = p.hops; nmylink = p.mylink; nm0 = p.m0;
                        osnr = -10.0 * log10(uniform_f64(g.ase) + uniform_f64(g.nli));
                        break;
                    }
                }
            }
            c.skip_id = -1;

            // ---- 4. provisioned as the step provisions: the new range, or the old one again
            const bool same = found && npath == old_path && nm == m && ns == s;
            if (!found || same) {
                int end = s + n;
                if (end < S) end += 1;
                move_mark_record<R32>(c, a, s, end, false);
                status = same ? 2 : refused ? 4 : 3;
                break;
            }
            int end = ns + nn;
            if (end < S) end += 1;
            mark_links<false>(c, nhops, nmylink, ns, end, false);
            if (lane == 0) {
                uint32_t ra, rb;
                rec_pack<R32>(npath, nm0, ns, nn, nm, ra, rb);
                c.sa[idx] = ra; c.sb[idx] = rb;                             // release time (and its sign) and id stay
                if (P.track_ids) {
                    c.e->osnr_flushed += osnr - c.so[idx];                  // the Service object is updated, as defragment() does
                    c.so[idx] = osnr;
                }
            }
            wave_sync();
            status = 0;
            moved++;
            new_action = nk * M * S + (M - 1 - nm) * S + ns;
            mrg = osnr - P.mod_thr[nm] - margin;
            delta = nn * uniform_i32(nhops) - n * old_hops;
        } while (false);

        if (lane < kMoveOut) {
            const double v[kMoveOut] = {(double)status, (double)idx, (double)old_action, (double)new_action, mrg, (double)delta};
            double r = v[0];
            for (int k = 1; k < kMoveOut; k++) r = lane == k ? v[k] : r;
            orow[(size_t)t * kMoveOut + lane] = r;
        }
    }

    if (!moved) return;                                                     // nothing stored: byte for byte as it was
    c.lane_terms = 0; c.gn_evals = 0; c.gn_skips = 0;                       // a move is no step: total_* stay
    c.paths_tried = 0; c.path_hops = 0; c.active_sum = 0;
    store_state(c);
}

}  // namespace ongym
