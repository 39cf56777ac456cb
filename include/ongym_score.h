/* ongym_score.h - a weighted candidate-scoring policy on device, the weights given per call and per replica.
 * Included by ongym.h (after its declarations); not meant to be included on its own.
 *
 * ongym_score_actions answers, for every replica's PENDING request, "which placement has the lowest w . x", where x are ten
 * features of a candidate placement and w is a weight vector of the caller's: one for all replicas or one per replica, so that a
 * whole population of heuristics is evaluated in one launch (K = k_paths, M = n_mods, S = n_slots, F = ONGYM_SCORE_FEATURES).
 *
 * Candidates  exactly those of ONGYM_POLICY_HIGHEST_SNR (heuristics.py:272-328): route k = 0..K-1 of the request's node pair,
 *             format m from the best (M - 1) down with a positive slot count n, every start s that `_get_candidates` accepts on
 *             the route's row (n free slots and a free guard slot, the guard waived when the block ends at S).  A candidate is
 *             FEASIBLE when its GSNR clears minimum_osnr[m] + the replica's margin, by the step's own decision.  GSNR is the
 *             value that policy computes, bit for bit, and so identical for two formats that share (route, s, n).
 * Features    x0 route        k
 *             x1 hops         hops of the route
 *             x2 format_rank  M - 1 - m (0 = the best format)
 *             x3 slots        n
 *             x4 slot_hops    n x hops
 *             x5 start        s
 *             x6 load         (S - free cells of the route row) / hops, the quantity of ONGYM_POLICY_LOAD_BALANCING
 *             x7 touch        0..2: 1 if s == 0 or cell s - 1 of the route row is not free, plus 1 if e == S or cell e is not
 *                             free, e = min(s + n + 1, S) (the cell behind the guard slot)
 *             x8 gsnr         dB
 *             x9 margin       gsnr - (minimum_osnr[m] + the replica's margin), dB
 * Score       t = w0 x0, then t = t + wf xf for f = 1..9: every product and every sum rounded on its own (no fused multiply-add).
 * Winner      the lowest score.  Candidates are walked k ascending, format best first, s ascending; a later candidate replaces
 *             the best so far only if score < best - 1e-12 x (|w8| + |w9|).  With w8 = w9 = 0 every feature is exact and the
 *             rule is a strict `<`: the first of equal scores wins.  With only w8 = -1 it is highest SNR's own tie rule.  (Like
 *             that policy the kernel takes the exact minimum of 64 consecutive starts at a time, first one on ties, and applies
 *             the band between such groups.)  A NaN score never wins.
 * weights     double [F] (per_replica == 0) or [batch][F].
 * actions     int32 [batch], required: k M S + (M - 1 - m) S + s of the winner, the step's action index; the reject action
 *             K M S where no candidate is feasible.  A replica without a pending request gets -1, as ongym_policy_actions gives.
 * best_out    double [batch][1 + F], optional: the winner's score and x0..x9; NaN where there is no winner.
 * count_out   int32 [batch][3], optional: candidates with spectrum; feasible candidates; flags - 0 with a winner, else
 *             ONGYM_F_BLOCKED_RESOURCES / ONGYM_F_BLOCKED_OSNR by highest SNR's rule (ONGYM_F_NO_REQUEST without a request).
 * Read-only: no replica state, statistic or counter changes.  Refused (ONGYM_E_ARG): NULL weights, NULL actions,
 * n_mods_consider < n_mods (no format window), a weight in a host array that is not finite (a device array is not
 * inspected); ONGYM_E_LIMIT: the LDS block (highest SNR's: the state block + 11 (2 S + 2) + 1024 bytes) exceeds 160 KiB.
 * Buffers: host buffers (staged through a device buffer grown on demand; the call synchronises once), or device buffers with
 * cfg.io_device (then the call only launches on the environment's stream and nothing synchronises; weights and best_out
 * 8-byte aligned).  ongym_last_kernel_ms times the kernel. */
#ifndef ONGYM_SCORE_H
#define ONGYM_SCORE_H

#define ONGYM_SCORE_FEATURES 10
int ongym_score_actions(ongym_env *env, const double *weights, int32_t per_replica,
                        int32_t *actions, double *best_out, int32_t *count_out);

#endif /* ONGYM_SCORE_H */
