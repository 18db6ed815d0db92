/*
 * fmhip_ranking.h — ranking evaluation with a trained factorization machine (libfmhip.so): where does a held-out item land
 * in a context's complete ranking, and the metrics that follow from it (HitRate@K, Recall@K, Precision@K, NDCG@K, MRR, MAP).
 *
 * fmhip_topk (fmhip_topk.h, which this header includes) answers "which K candidates rank highest"; it is capped at
 * FMHIP_TOPK_MAX and says nothing about a row outside the list.  fmhip_rank answers the evaluation question instead: for given
 * (context, relevant candidate row) pairs, the exact 0-based position of that row in the list fmhip_topk would return with
 * K = n_candidates.  It is the same sweep — one forward per row set, the [B x Kp] . [Kp x M] product on the exact-f32 MFMA —
 * with a compare-and-count in place of the list insertion: the B x M scores never exist in memory and nothing but integers
 * (and, if asked for, one score per relevant row) leaves the GPU.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws).
 *
 *  - threads: fmhip_rank is a SCORING call in the sense of fmhip.h — re-entrant, the model's lock taken shared, on a stream and
 *    in a workspace of its own, ordered behind whatever the model's own stream has queued.  fmhip_rank_metrics touches no GPU.
 *  - a lazily decayed model scores correctly; the scores do not depend on the model's loss or optimizer.
 *  - memory: the device workspace is O((B_chunk + M) * Kp + nq * splits + sum of the chunk's exclusions), nq = the chunk's
 *    (context, relevant row) pairs — never O(B * M).  Nothing is cached between calls.
 *  - cost: a context with several relevant rows is swept once PER ROW (every pair is a query of its own); a context without
 *    relevant rows costs nothing.  Exclusions cost one pair score per (context, excluded row) and one compare per
 *    (query, excluded row of its context); nothing is looked up inside the sweep.
 *  - determinism: a pair's score is fmhip_pair_scores' bit for bit, whatever tile, chunk or candidate split it falls into;
 *    ranks are integers counted from those bits, so results are identical run to run and batch to batch.
 */
#ifndef FMHIP_RANKING_H
#define FMHIP_RANKING_H
#include "fmhip_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rank[p], for p in [rel_ptr[c], rel_ptr[c+1]): the 0-based position of candidate row rel[p] in context c's COMPLETE ranking —
 * the list fmhip_topk would return with K = n_candidates: the number of candidates d, not excluded for c and d != rel[p],
 * with score(c,d) > score(c,rel[p]), or an equal score and d < rel[p]; NaN below -Inf, NaNs among themselves by row.
 * Other relevant items of the same context count as ordinary candidates.  score (nullable): score(c, rel[p]), the bits of
 * fmhip_pair_scores.
 * Datasets, FMHIP_ERR_SHAPE and FMHIP_ERR_INVALID as fmhip_topk (a NULL handle; one of excl_ptr / excl NULL and the other
 * not; excl_ptr negative or decreasing; an excluded number outside [0, n_candidates) or not ascending).  Also
 * FMHIP_ERR_INVALID: rel_ptr, rel or rank NULL while rel_ptr[n_contexts] > 0 (rel_ptr may be NULL only when n_contexts == 0);
 * rel_ptr negative or decreasing; a relevant row outside [0, n_candidates), or a context's list that is not ascending and
 * distinct; a row that is both relevant and excluded for the same context.  n_contexts == 0, rel_ptr[n_contexts] == 0 or
 * n_candidates == 0 (without relevant rows) is not an error: nothing is written. */
int fmhip_rank(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates,
               const int64_t *rel_ptr, const int32_t *rel,          /* [n_contexts+1], ascending & distinct per context */
               const int64_t *excl_ptr, const int32_t *excl,        /* nullable pair, as fmhip_topk */
               int32_t *rank, double *score);

typedef struct fmhip_rank_metrics { int32_t struct_size; int32_t k; int64_t contexts, skipped, relevant;
    double hit_rate, recall, precision, ndcg, mrr, map; } fmhip_rank_metrics_t;
/* (the typedef carries a _t: in C a typedef name and a function share one name space, and the function is fmhip_rank_metrics)
 * HOST ONLY (no GPU, like fmhip_auc_scores): the metrics of ranks as fmhip_rank returns them, cut at k >= 1.
 * The caller sets out->struct_size = sizeof(fmhip_rank_metrics_t).  Averages over the contexts that have at least one relevant row
 * (`contexts` of them; `skipped` the others; `relevant` = rel_ptr[n_contexts] - rel_ptr[0]); per context, with R its ranks:
 *   hit_rate   [min R < k]                         recall     #{r < k} / |R|              precision  #{r < k} / k
 *   ndcg       sum_{r < k} 1 / log2(r + 2)  over  sum_{j < min(|R|, k)} 1 / log2(j + 2)
 *   mrr        1 / (min R + 1), uncut              map        (1 / |R|) sum_j (j + 1) / (r_(j) + 1), ranks ascending, uncut
 * fp64 sums in context order; no evaluated context: every metric is 0.  FMHIP_ERR_INVALID: out NULL or a wrong struct_size;
 * k < 1; n_contexts < 0; rel_ptr NULL while n_contexts > 0, negative or decreasing; rank NULL while there are ranks; a negative
 * rank; two equal ranks within one context. */
int fmhip_rank_metrics(int64_t n_contexts, const int64_t *rel_ptr, const int32_t *rank, int32_t k, fmhip_rank_metrics_t *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_RANKING_H */
